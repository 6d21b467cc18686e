#!/usr/bin/env python3
"""Waits and counts of a kernel's MFMA region, from the compiler's assembly.

usage: isa_waits.py <file.hip of desco_amd/csrc> <kernel name> [--json]

Compiles the file device-only with the Makefile's HIPFLAGS (`--cuda-device-only -S`, into a temporary directory; needs
hipcc, no GPU), takes the kernel whose mangled name contains <kernel name>, and reports on the REGION between the first
and the last v_mfma of the innermost loop that holds MFMAs (the whole kernel body if no loop does):

  * MFMAs, LDS reads and writes inside / outside inline-asm blocks (the compiler brackets asm with ;;#ASMSTART /
    ;;#ASMEND), scalar memory loads, global loads and stores;
  * every s_waitcnt variant with its count;
  * for every LDS read of the region, the distance in MFMAs to the wait that COVERS it: LDS operations of a wave return
    in order, so a read is complete at the first s_waitcnt lgkmcnt(n) that has at least n LDS operations between the
    read and itself.  Reads whose destination feeds an MFMA's A / B operand are "operand" reads (a weight ring), the
    others "constant" reads; the shortest distance is reported per class.  A read that no wait of the region covers
    (requested for the next trip of the loop) counts the MFMAs up to the region's end, a lower bound.  The count is only
    meaningful if the region is straight-line code (reported as `branches`) and holds no scalar memory load (those
    return out of order and share the counter);
  * VGPRs, SGPR / VGPR spills and scratch bytes from the kernel's metadata.

It reports on waits and counts only."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "desco_amd", "csrc")

LDS_RD = re.compile(r"^ds_(read|load)\w*\s")
LDS_ANY = re.compile(r"^ds_\w+\s")
SMEM_LD = re.compile(r"^s_(load|buffer_load)_\w+\s")
VMEM_LD = re.compile(r"^(global|buffer|flat)_load\w*\s")
VMEM_ST = re.compile(r"^(global|buffer|flat)_(store|atomic)\w*\s")
MFMA = re.compile(r"^v_mfma_\w+\s")
WAIT = re.compile(r"^s_waitcnt\s+(.*)$")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\S+)")
LABEL = re.compile(r"^(\.?[A-Za-z_][\w.$]*):")
REG = re.compile(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b")


def hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def makefile_hipflags():
    """HIPFLAGS of desco_amd/csrc/Makefile (continuation lines joined, $(ARCH) expanded)"""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_asm(hip_file):
    src = hip_file if os.path.isabs(hip_file) or os.path.exists(hip_file) else os.path.join(CSRC, hip_file)
    with tempfile.TemporaryDirectory() as wd:
        out = os.path.join(wd, "kernel.s")
        cmd = [hipcc()] + makefile_hipflags() + ["-I", os.path.abspath(CSRC), "--cuda-device-only", "-S",
                                                 os.path.abspath(src), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=wd)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
        return open(out).read()


def kernel_body(text, kernel):
    """[(instruction text, in_asm, label or None)] of the first function whose symbol contains `kernel`"""
    lines = text.split("\n")
    start = sym = None
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w.$]*):", l)
        if m and kernel in m.group(1):
            start, sym = i + 1, m.group(1)
            break
    if start is None:
        raise RuntimeError(f"no kernel matching {kernel!r}")
    body, in_asm = [], False
    for l in lines[start:]:
        s = l.strip()
        if s.startswith(".Lfunc_end") or s.startswith("s_endpgm"):
            break
        if s.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            in_asm = False
            continue
        m = LABEL.match(s)
        if m:
            body.append(("", False, m.group(1)))
            continue
        s = s.split(";")[0].strip()
        if not s or s.startswith("."):
            continue
        body.append((s, in_asm, None))
    return sym, body


def metadata(text, sym):
    # the kernel's entry of amdhsa.kernels: the top-level list item that holds its .name
    block = ""
    for it in re.split(r"\n  - ", text[max(text.find("amdhsa.kernels"), 0):]):
        if re.search(r"\.name:\s+" + re.escape(sym) + r"\s", it):
            block = it
            break
    def field(name):
        f = re.search(r"\." + name + r":\s+(\d+)", block)
        return int(f.group(1)) if f else None
    return {"vgprs": field("vgpr_count"), "agprs": field("agpr_count"), "sgpr_spills": field("sgpr_spill_count"),
            "vgpr_spills": field("vgpr_spill_count"), "scratch_bytes": field("private_segment_fixed_size"),
            "lds_static_bytes": field("group_segment_fixed_size")}


def mfma_region(body):
    """(first, last, lo, hi): first / last MFMA of the innermost loop [lo, hi] that holds MFMAs"""
    labels = {lab: i for i, (_, _, lab) in enumerate(body) if lab}
    mf = [i for i, (s, _, _) in enumerate(body) if MFMA.match(s)]
    if not mf:
        raise RuntimeError("kernel has no MFMA")
    best = None
    for i, (s, _, _) in enumerate(body):
        m = BRANCH.match(s)
        if m and m.group(1) in labels and labels[m.group(1)] < i:           # a back edge: loop [target, i]
            lo, hi = labels[m.group(1)], i
            inside = [k for k in mf if lo <= k <= hi]
            if inside and (best is None or hi - lo < best[1] - best[0]):
                best = (lo, hi, inside)
    inside = best[2] if best else mf
    return inside[0], inside[-1], (best[0] if best else 0), (best[1] if best else len(body) - 1)


def vregs(operand):
    out = set()
    for m in REG.finditer(operand):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def analyse(text, kernel):
    sym, body = kernel_body(text, kernel)
    first, last, lo, hi = mfma_region(body)
    reg = [b for b in body[first:last + 1] if not b[2]]
    res = {"kernel": sym, "mfma": 0, "lds_reads_asm": 0, "lds_reads_compiler": 0, "lds_writes_asm": 0,
           "lds_writes_compiler": 0, "scalar_loads": 0, "global_loads": 0, "global_stores": 0, "branches": 0, "waits": {}}
    for s, in_asm, _ in reg:
        if MFMA.match(s):
            res["mfma"] += 1
        elif LDS_RD.match(s):
            res["lds_reads_asm" if in_asm else "lds_reads_compiler"] += 1
        elif LDS_ANY.match(s):
            res["lds_writes_asm" if in_asm else "lds_writes_compiler"] += 1
        elif SMEM_LD.match(s):
            res["scalar_loads"] += 1
        elif VMEM_LD.match(s):
            res["global_loads"] += 1
        elif VMEM_ST.match(s):
            res["global_stores"] += 1
        elif BRANCH.match(s):
            res["branches"] += 1
        w = WAIT.match(s)
        if w:
            key = " ".join(w.group(1).split())
            res["waits"][key] = res["waits"].get(key, 0) + 1
    res["lgkmcnt0_waits"] = sum(n for k, n in res["waits"].items() if re.search(r"lgkmcnt\(0\)", k))

    # operand reads: the destination is an A / B operand of a later MFMA before it is overwritten.  Followed through
    # the whole loop body (a read of the region's end may feed the next trip: two trips), in layout order.
    loop = [(k, b[0]) for k, b in enumerate(body[lo:hi + 1], lo) if not b[2]]
    index_in_reg = {}
    k2 = 0
    for k, b in enumerate(body[first:last + 1], first):
        if not b[2]:
            index_in_reg[k] = k2
            k2 += 1
    owner, operand_reads = {}, set()
    for trip in range(2):
        for k, s in loop:
            ops = s.split(None, 1)[1].split(",") if " " in s else []
            if MFMA.match(s):
                for o in ops[1:3]:
                    for r in vregs(o):
                        if r in owner:
                            operand_reads.add(owner[r])
                for r in vregs(ops[0]):
                    owner.pop(r, None)
            elif LDS_RD.match(s):
                for r in vregs(ops[0]):
                    owner[r] = index_in_reg.get(k, -1)
            elif ops and (s.startswith("v_") or VMEM_LD.match(s)):
                for o in ops[:2 if "swap" in s.split()[0] else 1]:
                    for r in vregs(o):
                        owner.pop(r, None)
    # covering wait of every read
    dist = {"operand": [], "constant": []}
    uncovered = {"operand": 0, "constant": 0}
    for i, (s, _, _) in enumerate(reg):
        if not LDS_RD.match(s):
            continue
        younger = mf = 0
        cover = None
        for s2, _, _ in reg[i + 1:]:
            if MFMA.match(s2):
                mf += 1
            elif LDS_ANY.match(s2):
                younger += 1
            w = WAIT.match(s2)
            if w:
                c = re.search(r"lgkmcnt\((\d+)\)", w.group(1))
                if c and int(c.group(1)) <= younger:
                    cover = mf
                    break
                if c is None and "vmcnt" not in w.group(1) and "expcnt" not in w.group(1):   # s_waitcnt 0
                    cover = mf
                    break
        cls = "operand" if i in operand_reads else "constant"
        if cover is None:
            uncovered[cls] += 1
            cover = mf
        dist[cls].append(cover)
    res["operand_reads"] = len(dist["operand"])
    res["constant_reads"] = len(dist["constant"])
    res["min_mfma_operand_read_to_wait"] = min(dist["operand"]) if dist["operand"] else None
    res["min_mfma_constant_read_to_wait"] = min(dist["constant"]) if dist["constant"] else None
    res["reads_covered_beyond_region"] = uncovered
    res.update(metadata(text, sym))
    return res


def report(hip_file, kernel):
    return analyse(compile_asm(hip_file), kernel)


def main():
    args = [a for a in sys.argv[1:] if a != "--json"]
    if len(args) != 2:
        print(__doc__)
        return 2
    res = report(args[0], args[1])
    if "--json" in sys.argv:
        print(json.dumps(res))
        return 0
    print(f"{args[0]}: {res['kernel']}")
    print(f"  region: {res['mfma']} MFMAs, {res['branches']} branches, {res['scalar_loads']} scalar loads, "
          f"{res['global_loads']} global loads, {res['global_stores']} global stores")
    print(f"  LDS reads: {res['lds_reads_asm']} in asm blocks, {res['lds_reads_compiler']} outside;  "
          f"LDS writes: {res['lds_writes_asm']} in asm blocks, {res['lds_writes_compiler']} outside")
    print("  waits: " + (", ".join(f"{n} x s_waitcnt {k}" for k, n in sorted(res["waits"].items())) or "none"))
    print(f"  lgkmcnt(0) waits: {res['lgkmcnt0_waits']}")
    print(f"  MFMAs from a read to the wait that covers it, shortest: operand reads ({res['operand_reads']}) "
          f"{res['min_mfma_operand_read_to_wait']}, constant reads ({res['constant_reads']}) "
          f"{res['min_mfma_constant_read_to_wait']};  covered beyond the region: {res['reads_covered_beyond_region']}")
    print(f"  VGPRs {res['vgprs']}, AGPRs {res['agprs']}, VGPR spills {res['vgpr_spills']}, SGPR spills {res['sgpr_spills']}, "
          f"scratch {res['scratch_bytes']} B")
    return 0


if __name__ == "__main__":
    sys.exit(main())
