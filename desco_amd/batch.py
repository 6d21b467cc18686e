"""Device-resident batch containers (replace PyG ``HeteroData``/``Data`` batches on the hot path).

The reference moves a collated ``HeteroData`` to the GPU per batch (Lightning) and the model reads
``node_feature_dict`` / ``edge_index_dict`` (gnn_model.py:60-63).  Here a batch is a handful of
flat int32/fp32 tensors in HBM in the layout the kernels consume; the PyG-style dict views are
kept as (lazy, host-side) properties for interop and tests.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .graphs import GraphSet
from .partition import NeighborhoodPartition


def _norm_device(device) -> torch.device:
    """torch.device("cuda") and torch.device("cuda:0") compare unequal; always carry the index."""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _i32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)


# NeighborhoodBatch._level_csr
_LevelCSR = namedtuple("_LevelCSR", "col low csrc qsrc start tdeg dmax cstart ctdeg cdmax deg pos")
_CanonTables = namedtuple("_CanonTables", "uptr1 levels size offset anchor_rows")
_PoolClasses = namedtuple("_PoolClasses", "pcls prep rep_ptr bits slot nslots anch_row")


def _transpose_index(vrowptr: np.ndarray, vcol: np.ndarray, n_src: int):
    """For every source row, the virtual rows that read it (the index of the backward gather)."""
    cnt = np.diff(vrowptr.astype(np.int64))
    vrow_of_edge = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    src = vcol.astype(np.int64)
    order = np.argsort(src, kind="stable")
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n_src))])
    return t_rowptr, vrow_of_edge[order]


class _TrainIndexMixin:
    """Lazily built device indices the backward pass needs (transposed CSR, segment ids)."""

    def train_index(self):
        if getattr(self, "_train_index", None) is None:
            from . import ops
            # both built on the device (desco_vcsr_transpose_sym / desco_segment_ids): the blocks
            # are symmetric, so the transposed index is row-local (include/desco_hip.h)
            num_count = getattr(self, "num_count", self.num_rows)
            t_rowptr, t_col = ops.vcsr_transpose_sym(self.vrowptr, self.vcol, self.num_rows,
                                                     self.slots, num_count)
            seg_ptr = self._seg_ptr_device()
            n_seg_rows = num_count if self.slots == 4 else self.num_rows
            seg_id = ops.segment_ids(seg_ptr, n_seg_rows)
            dev = self.vrowptr.device
            S = self.slots
            self._train_index = {
                "t_rowptr": t_rowptr, "t_col": t_col, "seg_id": seg_id,
                "ident_ptr": torch.arange(n_seg_rows + 1, device=dev, dtype=torch.int32),
                # the same transposed index for gradient rows laid out [row][S + 1 blocks of 64] (S relation
                # slots + the self block, one GEMM output of the fused training trunk): virtual row
                # k S + s -> k (S + 1) + s
                "t_col_s1": (t_col + torch.div(t_col, S, rounding_mode="floor")).to(torch.int32),
            }
        return self._train_index


    def plain_csr(self):
        """(rowptr [num_rows + 1], col): the PLAIN CSR of the block -- one entry per row, the union of the row's relation
        slots, which is all its neighbours (a homogeneous model reads it: plain_forward).  A strided read of the
        virtual-row pointer, made once per batch.  The blocks are symmetric, so this is also its own transposed index."""
        c = self.__dict__.get("_plain_csr")
        if c is None:
            c = self.__dict__["_plain_csr"] = (self.vrowptr[::self.slots].contiguous(), self.vcol)
        return c


class NeighborhoodBatch(_TrainIndexMixin):
    """B canonical neighborhoods: N_c count rows followed by B canonical rows, 4-slot CSR."""

    slots = 4

    def __init__(self, part: NeighborhoodPartition, device, node_feature: Optional[torch.Tensor] = None,
                 y: Optional[torch.Tensor] = None, input_dim: int = 1, anchor_flag: bool = False):
        """``anchor_flag``: the batch of a homogeneous model (NeighborhoodDataset(hetero_graph=False)) -- ``node_feature``
        [num_rows, 1] is 0 on the count rows and 1 on the canonical rows (get_neigh_canonical, data.py:369-371), made on
        ``device`` (and made again there by ``to``: never uploaded)."""
        self.part = part
        self.device = _norm_device(device)
        device = self.device
        self.num_graphs = part.num_neigh
        self.num_count = part.num_count
        self.num_rows = part.num_rows
        da = getattr(part, "device_arrays", None)
        if da is not None and _norm_device(da["device"]) == device:    # built on this device already
            self.count_ptr, self.vrowptr, self.vcol = da["count_ptr"], da["vrowptr"], da["vcol"]
        else:
            self.count_ptr = _i32(part.count_ptr, device)
            self.vrowptr = _i32(part.vrowptr, device)
            self.vcol = _i32(part.vcol, device)
        self.input_dim = input_dim if node_feature is None else node_feature.shape[1]
        # None == all-zero features (ZeroNodeFeat, workload.py:431-440): pre_mp output is its bias
        self.node_feature = None if node_feature is None else node_feature.to(device).float()
        self.anchor_flag = bool(anchor_flag)
        if self.anchor_flag:
            if node_feature is not None:
                raise ValueError("NeighborhoodBatch: anchor_flag makes node_feature itself; pass none")
            self.input_dim = 1
            self.node_feature = torch.zeros((self.num_rows, 1), device=device)
            self.node_feature[self.num_count:] = 1.0
        self.y = None if y is None else y.to(device)

    def to(self, device):
        if _norm_device(device) == self.device:
            return self
        if self.anchor_flag:
            return NeighborhoodBatch(self.part, device, None, self.y, 1, anchor_flag=True)
        return NeighborhoodBatch(self.part, device, self.node_feature, self.y, self.input_dim)

    def _seg_ptr_host(self):
        return self.part.count_ptr.astype(np.int64)

    def _seg_ptr_device(self):
        return self.count_ptr

    def _pool_on_device(self) -> bool:
        """The pooling index is built by desco_pool_index_dev only when this batch holds a device ``count_ptr`` on a
        cuda device (``DESCO_DEVICE_PROLOGUE=0`` / ``device_prologue = False``: the numpy path on the host copy)."""
        cp = self.__dict__.get("count_ptr")
        on = self.__dict__.get("device_prologue")
        if on is None:
            import os
            on = os.environ.get("DESCO_DEVICE_PROLOGUE", "1") != "0"
        return bool(on) and isinstance(cp, torch.Tensor) and cp.is_cuda

    def _pool_dev(self):
        """(bits, slot, num_slots, largest, smallest neighborhood) from the device; one read-back, cached"""
        r = self.__dict__.get("_pool_dev_result")
        if r is None:
            from . import ops
            B = int(self.count_ptr.numel()) - 1
            nc = self.__dict__.get("num_count")
            if nc is None:
                nc = self.part.num_count
            bits, slot, totals = ops.pool_index_dev(self.count_ptr, B, nc)
            ns, mx, mn, _ = totals.tolist() if B else (0, 0, 1, 0)
            r = self.__dict__["_pool_dev_result"] = (bits, slot, int(ns), int(mx), int(mn))
        return r

    def max_count_rows(self) -> int:
        """the largest number of count rows of a neighborhood of this batch (cached)"""
        m = self.__dict__.get("_max_count_rows")
        if m is None:
            if self._pool_on_device():
                m = self._pool_dev()[3]
            else:
                d = np.diff(self.part.count_ptr)
                m = int(d.max()) if len(d) else 0
            self.__dict__["_max_count_rows"] = m
        return m

    def pool_index(self):
        """(pool_bits, pool_slot, num_slots) of the fused pooling (desco_shmp_layer_pool_f16x3_f32 and its bf16x6 twin):
        per 16-row wave tile of the layer kernel, the bitmap of count rows that END a neighborhood and the first partial
        slot of the tile (a tile uses one slot per neighborhood that has a row in it)."""
        idx = self.__dict__.get("_pool_index")
        if idx is None and self._pool_on_device():
            bits, slot, ns, _, mn = self._pool_dev()
            if mn <= 0:
                raise ValueError("fused pooling needs at least one count row per neighborhood")
            if ns >= 2 ** 31:
                raise ValueError("too many pooling slots for int32")
            idx = self.__dict__["_pool_index"] = (bits, slot, ns)
        if idx is None:
            TR = 16
            cp = self.part.count_ptr.astype(np.int64)
            nc = int(cp[-1])
            if (np.diff(cp) <= 0).any():
                raise ValueError("fused pooling needs at least one count row per neighborhood")
            nt = (nc + TR - 1) // TR
            ends = cp[1:] - 1
            bits = np.zeros(nt, dtype=np.uint32)
            np.bitwise_or.at(bits, ends // TR, (np.uint32(1) << (ends & (TR - 1)).astype(np.uint32)))
            pop = np.zeros(nt, dtype=np.int64)
            np.add.at(pop, ends // TR, 1)
            last_row = np.minimum(TR * np.arange(nt, dtype=np.int64) + TR - 1, nc - 1)
            carry = ((bits >> (last_row & (TR - 1)).astype(np.uint32)) & 1) == 0    # a segment runs on into the next tile
            nseg = pop + carry
            slot = np.concatenate([[0], np.cumsum(nseg)])
            if slot[-1] >= 2 ** 31:
                raise ValueError("too many pooling slots for int32")
            dev = self.device
            idx = self.__dict__["_pool_index"] = (torch.from_numpy(bits.view(np.int32)).to(dev),
                                                   torch.from_numpy(slot[:-1].astype(np.int32)).to(dev), int(slot[-1]))
        return idx

    def degree_table_index(self, max_rows: int = 1 << 16):
        """The count rows' S slot degrees as an index into their DISTINCT tuples (built once per batch, on the device):
        ``(uptr, row_id, vcol_t)`` or None.  The closed-form first layer (ZeroNodeFeat: every node of a type has the same
        input row) makes X_1[i] a function of row i's degree tuple alone, so X_1 = T[row_id] for the table T of the U
        distinct tuples -- ``uptr`` [U S + 1] int32 is their row-pointer array (what desco_degree_affine_f32 turns into
        T), ``row_id`` [num_count] int32 each count row's table row, and ``vcol_t`` = vcol with the sources of the
        relation slots 0 and 1 (count rows) replaced by their table rows, so that the second layer's launches gather
        from T (desco_shmp_layer_pool_table_f16x3_f32, which recomputes the launch's own rows from their degrees).  None when the batch has more than ``max_rows`` distinct tuples
        (the table must stay cache-resident to pay)."""
        return self._table_indices(max_rows)[0]

    def _table_indices(self, max_rows: int = 1 << 16):
        """(degree_table_index, canonical_table_index): built together, once per batch"""
        if "_degree_table" in self.__dict__:
            return self.__dict__["_degree_table"]
        res = ctab = None
        S, nc, n = self.slots, self.num_count, self.num_rows
        if S == 4 and nc > 0:
            vr = self.vrowptr.to(torch.int64)
            deg = (vr[1:] - vr[:-1]).view(n, S)
            dc = deg[:nc]
            m = int(dc.max().item()) + 1
            if m ** S < 2 ** 62:
                key = ((dc[:, 0] * m + dc[:, 1]) * m + dc[:, 2]) * m + dc[:, 3]
                uniq, inv = torch.unique(key, return_inverse=True)
                if uniq.numel() <= max_rows:
                    ut = torch.stack([uniq // (m ** 3), (uniq // (m ** 2)) % m, (uniq // m) % m, uniq % m], dim=1)
                    uptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=ut.device), ut.reshape(-1).cumsum(0)])
                    # slot of every CSR entry: entry e belongs to (row, slot) pair rs(e); sources of slots 0, 1 are count rows
                    rs = torch.repeat_interleave(torch.arange(n * S, device=vr.device), deg.reshape(-1))
                    col = self.vcol.to(torch.int64)
                    low = (rs % S) < 2
                    if bool((col[low] < nc).all()):
                        row_id = inv.to(torch.int32)
                        vcol_t = torch.where(low, inv[col.clamp(max=nc - 1)], col).to(torch.int32)
                        res = (uptr.to(torch.int32).contiguous(), row_id.contiguous(), vcol_t.contiguous())
                        ctab = self._canonical_table(deg[nc:], low, col, vcol_t, max_rows)
        self.__dict__["_degree_table"] = (res, ctab)
        return res, ctab

    def _canonical_table(self, dq, low, col, vcol_t, max_rows):
        """``canonical_table_index`` from the intermediates of ``degree_table_index``: ``dq`` [B, S] the canonical rows'
        slot degrees, ``low`` / ``col`` per CSR entry (slot < 2; source id), ``vcol_t`` the count-slot remap"""
        nc, n, S = self.num_count, self.num_rows, self.slots
        if n <= nc:
            return None
        m = int(dq.max().item()) + 1
        if m ** S >= 2 ** 62:
            return None
        key = dq[:, 0]
        for s in range(1, S):
            key = key * m + dq[:, s]
        uniq, inv = torch.unique(key, return_inverse=True)
        if uniq.numel() > max_rows or not bool(((col >= nc) | low).all()):
            return None
        ut = torch.stack([(uniq // (m ** (S - 1 - s))) % m for s in range(S)], dim=1)
        uptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=ut.device), ut.reshape(-1).cumsum(0)])
        vcol_tc = torch.where(low, vcol_t.to(torch.int64), inv[(col - nc).clamp(min=0)]).to(torch.int32)
        return (uptr.to(torch.int32).contiguous(), inv.to(torch.int32).contiguous(), vcol_tc.contiguous())

    def canonical_table_index(self):
        """``degree_table_index`` once more for the CANONICAL rows (built with it, once per batch): ``(uptr_c, canon_id,
        vcol_tc)`` or None.  Under ZeroNodeFeat the first-layer canonical rows are a function of their slot degrees too, so
        the second layer's canonical->count table product has one distinct row per distinct tuple -- a dozen on molecule
        shapes: ``uptr_c`` [U_c S + 1] is the row-pointer array of the U_c distinct tuples (input of
        desco_degree_affine_f32), ``canon_id`` [B] each canonical row's tuple, and ``vcol_tc`` = ``vcol_t`` with the sources
        of the two TABLE slots (canonical rows) replaced by their tuple ids as well, so that the second layer's count
        launch reads ``ytab`` [U_c, .] with ``ytab_row0 = 0``.  None when ``degree_table_index`` is None or the canonical
        rows have too many distinct tuples."""
        return self._table_indices()[1]

    # eligibility bounds of layer2_table_index: a 16-row tile of rows of total degree <= 8 stages all its source ids (the
    # layer kernel's gather order is then a function of the row alone); a [16384, 64] fp32 table is 4 MiB, one XCD's L2
    LAYER2_MAX_DEGREE = 8
    LAYER2_MAX_CLASSES = 1 << 14
    LAYER2_MIN_ROWS_PER_CLASS = 8
    # ... and of gnn_model.SECOND_LAYER_GATHER (the third layer gathering from that table, X_2's count rows never written): what
    # it saves is the store and the read-back of X_2, which reach HBM only where the tensor outgrows the 256 MB memory-side
    # cache -- below 2^18 count rows (64 MiB) the pass measures the same either way (real-size COX2, 130 022 rows: replayed pass
    # 0.760 against 0.762 ms), and the rows stay where a caller can look at them.  About profit only, like the bound above
    LAYER2_GATHER_MIN_ROWS = 1 << 18
    # ... and of gnn_model.POOL_TABLES (the partial sums of X_1 and X_2 from one walk with both tables in LDS): every block of
    # that launch -- one per CU -- first copies the tables, up to 156 KiB each time, about 40 MB through L2 in all, a fixed
    # ten microseconds or so; what the walk saves grows with the rows, about 0.03 us per thousand (0.27 ms on 8.3 M), and
    # passes that cost near 2^18 count rows.  Smaller blocks keep the two launches.  About profit only
    POOL_TABLES_MIN_ROWS = 1 << 18

    def layer2_table_index(self):
        """The count rows' classes under the SECOND layer (built once per batch, on the batch's device): ``(cls, rep_uptr,
        rep_vcol, vcol_2)`` or None.  With the first layer a table of degree tuples (``degree_table_index``,
        ``canonical_table_index``), the second layer's count row i is a function of its four slot degrees and of its remapped
        CSR segment ``vcol_tc`` -- table ids, the same in whichever neighborhood the row sits -- so rows that agree in both get
        bit-equal X_2 rows: ``cls`` [num_count] int32 is each count row's class (exact: iterated pair refinement,
        ``_refine_classes``, no hashing), ``rep_uptr`` [U_2 S + 1] / ``rep_vcol`` the compact 4-slot CSR of one
        representative per class (its lowest row; the segment copied from ``vcol_tc``), on which the layer runs, and ``vcol_2``
        = ``vcol`` with the sources of slots 0 and 1 replaced by their class.  None unless the block has an empty table slot
        (``table_empty``) and both first-layer tables, no count row has more than 8 sources (tested before any sort), U_2 <=
        16384 and 8 U_2 <= num_count (the LAYER2_* bounds above; the last one is about profit only, and tests on small
        blocks lower it on their batch object)."""
        if "_layer2_table" in self.__dict__:
            return self.__dict__["_layer2_table"]
        self.__dict__["_layer2_table"] = res = self._build_layer2_table()
        if res is not None and res[0].is_cuda:
            from . import ops
            # the classes address the table of the representatives' rows in two kernels (desco_table_rows_pool_f32 and the
            # third layer's gather, desco_shmp_layer_selfidx_f16x3_f32): checked once per batch, here where they are built
            ops.index_range_check(res[0], (res[1].numel() - 1) // self.slots)
        return res

    def _level_csr(self):
        """what every table level reads of the block's CSR, whatever the level: per entry ``low`` (the source is a count row:
        slots 0 and 1) and the source as a count row ``csrc`` / as a canonical row ``qsrc`` (clamped; ``low`` says which one
        holds), per count row its segment ``start`` / ``tdeg`` (the longest: ``dmax``) and slot degrees ``deg``, per canonical
        row ``cstart`` / ``ctdeg`` (``cdmax``), and ``pos`` = 0 .. dmax - 1.  None where a count row has more than
        LAYER2_MAX_DEGREE sources (dense graphs leave here, before any sort)"""
        S, nc, n = self.slots, self.num_count, self.num_rows
        vr = self.vrowptr.to(torch.int64)
        start = vr[0:S * nc:S]
        tdeg = vr[S:S * nc + 1:S] - start                       # total degree of every count row
        dmax = int(tdeg.max().item())
        if dmax > self.LAYER2_MAX_DEGREE:
            return None
        dev = vr.device
        col = self.vcol.to(torch.int64)
        dall = vr[1:] - vr[:-1]
        low = (torch.repeat_interleave(torch.arange(n * S, device=dev), dall) % S) < 2
        cstart = vr[S * nc:S * n:S]
        ctdeg = vr[S * nc + S::S] - cstart
        return _LevelCSR(col, low, col.clamp(max=nc - 1), (col - nc).clamp(min=0, max=max(n - nc - 1, 0)), start, tdeg, dmax,
                         cstart, ctdeg, int(ctdeg.max().item()) if n > nc else 0, dall[:S * nc].view(nc, S),
                         torch.arange(max(dmax, 1), device=dev))

    @staticmethod
    def _rep_csr(c, rep, ent):
        """(rep_uptr, rep_vcol): the compact CSR of the count rows ``rep``, their segments copied from ``ent``"""
        rep_uptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=rep.device), c.deg[rep].reshape(-1).cumsum(0)])
        ne = ent.numel()
        if not ne:
            return rep_uptr, ent
        idx = c.start[rep][:, None] + c.pos[None, :]
        return rep_uptr, ent[idx.clamp(max=ne - 1)][c.pos[None, :] < c.tdeg[rep][:, None]]

    def _build_layer2_table(self):
        S, nc = self.slots, self.num_count
        if nc == 0 or not self.table_empty:                     # (the narrow-table case only: a table slot without entries)
            return None
        c = self._level_csr()
        if c is None:
            return None
        tab1, ctab = self._table_indices()
        if tab1 is None or ctab is None:
            return None
        # rows of one class agree in their degree tuple and in their segment of table ids (the slot boundaries inside the
        # segment follow from the degree tuple)
        vcol_tc = ctab[2].to(torch.int64)
        r = self._refine_classes(tab1[1].to(torch.int64), tab1[0].numel() // S, c.start, c.tdeg, vcol_tc, c.dmax,
                                 (int(vcol_tc.max().item()) + 2) if vcol_tc.numel() else 1,
                                 min(self.LAYER2_MAX_CLASSES, nc // self.LAYER2_MIN_ROWS_PER_CLASS))
        if r is None:
            return None
        key, u2 = r
        rep_uptr, rep_vcol = self._rep_csr(c, self._lowest_rows(key, u2), vcol_tc)
        vcol_2 = torch.where(c.low, key[c.csrc], c.col).to(torch.int32)
        i32 = lambda t: t.to(torch.int32).contiguous()
        return (i32(key), i32(rep_uptr), i32(rep_vcol), vcol_2.contiguous())

    def _table_level(self, level: int):
        """the class index of table level ``level`` >= 2 (``layer2_table_index``, ``layer3_table_index``, an entry of
        ``deep_table_index``), or None"""
        if level <= 3:
            return self.layer2_table_index() if level == 2 else self.layer3_table_index()
        deep = self.deep_table_index()
        return deep[level - 4] if level - 4 < len(deep) else None

    def rep_pool_index(self, level: int):
        """the fused-pooling index of ONE segment over the representatives of table level ``level`` (the pooled layer launch
        that computes their rows wants one; its partial rows are discarded): (pool_bits, pool_slot, a [slots, 64] buffer for
        them), cached per level"""
        cache = self.__dict__.setdefault("_rep_pool", {})
        idx = cache.get(level)
        if idx is None:
            u = (self._table_level(level)[1].numel() - 1) // self.slots
            nt = (u + 15) // 16
            dev = self.vrowptr.device
            bits = torch.zeros(nt, dtype=torch.int32, device=dev)
            bits[nt - 1] = 1 << ((u - 1) % 16)
            idx = cache[level] = (bits, torch.arange(nt, dtype=torch.int32, device=dev), torch.empty((nt, 64), device=dev))
        return idx

    # eligibility bounds of layer3_table_index, the path's own (tests lower LAYER2_* on small blocks and pin their launches): a
    # [16384, 64] fp32 table is one XCD's L2; fewer than 8 rows per class leave too little to save (MUTAG shapes: 3.5)
    LAYER3_MAX_CLASSES = 1 << 14
    LAYER3_MIN_ROWS_PER_CLASS = 8
    # ... and of gnn_model.THIRD_LAYER_TABLE as a whole: what it saves -- the store and the read-back of X_3, all but U_3 rows
    # of the third layer's count launch -- grows with the rows, what it adds (a 12 k-row launch, a third table in the pooling
    # walk, a gather of the canonical representatives) does not.  Measured break-even on COX2-shaped blocks between 390 066
    # count rows (neighborhood model +0.024 ms, 1.050 against 1.026) and 520 088 (-0.080 ms, 1.245 against 1.325), 780 132:
    # -0.12 ms (profiles/layer3_table_ab.md); the next power of two above it.  Smaller blocks -- the real-size COX2 pass, the
    # blocks on which tests pin the launches of the LAYER2_* paths -- do not build the index.  About profit only
    LAYER3_MIN_ROWS = 1 << 19

    @staticmethod
    def _refine_classes(key, nkey, start, tdeg, ent, dmax, width, umax):
        """pair refinement of the classes ``key`` (ids below ``nkey``) by the rows' ordered segments: rows of one class in the
        result agree in ``key`` and in ``ent[start : start + tdeg]`` (entries in [0, width - 1); a position past the row's end
        counts as -1).  As many segment positions per sorted ``torch.unique`` as fit a 62-bit key; exact, no hashing.
        -> (key, nkey), or None as soon as there are more than ``umax`` classes"""
        ne = ent.numel()
        j = 0
        while j < dmax:
            if nkey > umax:
                return None
            packed, bound = key, nkey
            while j < dmax and bound * width < 2 ** 62:
                e = torch.where(tdeg > j, ent[(start + j).clamp(max=max(ne - 1, 0))] + 1, torch.zeros_like(tdeg))
                packed, bound, j = packed * width + e, bound * width, j + 1
            assert bound > nkey, "a segment entry does not fit the key"
            uniq, key = torch.unique(packed, return_inverse=True)
            nkey = uniq.numel()
        return None if nkey > umax else (key, nkey)

    @staticmethod
    def _lowest_rows(key, nkey):
        """the lowest row of every class: the first of its run in a STABLE sort by class"""
        order = torch.argsort(key, stable=True)
        size = torch.bincount(key, minlength=nkey)
        return order[torch.cumsum(size, 0) - size]

    def layer3_table_index(self):
        """The count rows' classes under the THIRD layer (built once per batch, on the batch's device): ``(cls3, rep_uptr,
        rep_vcol, rep_self, vcol_3, ccls2, crep)`` or None; defined only where ``layer2_table_index`` is.

        The canonical rows of X_2 are a function of their degree tuple (``canon_id``) and their ordered segment of first-layer
        table ids (``vcol_tc``): ``ccls2`` [B] int32 is each canonical row's class under that pair and ``crep`` [U_c2] int64 the
        lowest canonical row of each class (an index into the B canonical rows).  A count row of X_3 is a function of its
        own X_2 row (``cls2``) and, per CSR entry in order, of the source's X_2 row: ``cls2[src]`` in slots 0 and 1,
        ``ccls2[src - num_count]`` in the table slots.  ``cls3`` [num_count] int32 is the class under that tuple (exact: the
        segment packed into 62-bit keys, one sorted ``torch.unique`` per key word), ``rep_uptr`` [U_3 S + 1] / ``rep_vcol`` the
        compact 4-slot CSR of one representative per class (its lowest row) with the sources remapped as above -- table2 rows in
        slots 0 and 1, rows of the [U_c2, 64] table product in the table slots -- ``rep_self`` [U_3] the representatives'
        ``cls2`` (their own rows in table2), and ``vcol_3`` = ``vcol`` with the sources of slots 0 and 1 replaced by ``cls3``
        (the fourth layer gathers from the table of X_3's distinct rows).  None unless the canonical rows, too, have at most 8
        sources (their gather order is then a function of the row alone as well), U_3 <= LAYER3_MAX_CLASSES,
        LAYER3_MIN_ROWS_PER_CLASS U_3 <= num_count and num_count >= LAYER3_MIN_ROWS (the last two about profit only; tests on
        small blocks lower them on their batch object)."""
        if "_layer3_table" in self.__dict__:
            return self.__dict__["_layer3_table"]
        self.__dict__["_layer3_table"] = res = self._build_layer3_table()
        if res is not None:
            self._check_level_ids(res, (self.layer2_table_index()[1].numel() - 1) // self.slots)
        return res

    @staticmethod
    def _check_level_ids(level, u_prev):
        """every id of a level's tuple that a kernel uses as an address, checked once per batch against the sizes of the level
        before it (``u_prev`` rows in its table): the classes (this level's table: the pooling walk, the next layer's own
        rows), the representatives' own rows and sources (the table before, the table product), the canonical classes"""
        cls_k, _, rep_vcol, rep_self, _, ccls, crep = level
        if cls_k.is_cuda:
            from . import ops
            ops.index_range_check(cls_k, rep_self.numel())
            ops.index_range_check(rep_self, u_prev)
            ops.index_range_check(rep_vcol, max(u_prev, crep.numel()))
            ops.index_range_check(ccls, crep.numel())

    def _next_level(self, c, key, u, ckey, uc, ent, ebound, umax):
        """One step of the recurrence that every level k >= 3 shares: ``key`` the count classes of X_{k-1} (``u`` of them),
        ``ckey`` the canonical classes of X_{k-2} (``uc``), ``ent`` per CSR entry the source's class of X_{k-2} -- the count
        class in slots 0 and 1, the canonical class in the table slots, ids below ``ebound`` -- and ``c`` = ``_level_csr()``.
        -> level k's tuple as ``layer3_table_index`` lays it out, or None where level k has more than ``umax`` classes"""
        # canonical classes of X_{k-1}: the own class, then per entry the source's class
        ckey, uc = self._refine_classes(ckey, uc, c.cstart, c.ctdeg, ent, c.cdmax, ebound + 1, ckey.numel())
        crep = self._lowest_rows(ckey, uc)
        # count classes of X_k: the same one level on
        ent = torch.where(c.low, key[c.csrc], ckey[c.qsrc])
        r = self._refine_classes(key, u, c.start, c.tdeg, ent, c.dmax, max(u, uc) + 1, umax)
        if r is None:
            return None
        key_k, u_k = r
        rep = self._lowest_rows(key_k, u_k)
        rep_uptr, rep_vcol = self._rep_csr(c, rep, ent)
        vcol_k = torch.where(c.low, key_k[c.csrc], c.col).to(torch.int32)
        i32 = lambda t: t.to(torch.int32).contiguous()
        return (i32(key_k), i32(rep_uptr), i32(rep_vcol), i32(key[rep]), vcol_k.contiguous(), i32(ckey), crep.contiguous())

    def _build_layer3_table(self):
        S, nc, n = self.slots, self.num_count, self.num_rows
        tab2 = self.layer2_table_index() if nc >= self.LAYER3_MIN_ROWS else None    # (small blocks leave before any work)
        if tab2 is None or n == nc:
            return None
        c = self._level_csr()
        if c.cdmax > self.LAYER2_MAX_DEGREE:
            return None
        # level 3 from the first layer's tables: canonical classes of X_1 = degree tuples, entries = first-layer table ids
        tab1, ctab = self._table_indices()
        u1, uc1 = tab1[0].numel() // S, (ctab[0].numel() - 1) // S
        return self._next_level(c, tab2[0].to(torch.int64), (tab2[1].numel() - 1) // S, ctab[1].to(torch.int64), uc1,
                                ctab[2].to(torch.int64), max(u1, uc1),
                                min(self.LAYER3_MAX_CLASSES, nc // self.LAYER3_MIN_ROWS_PER_CLASS))

    # eligibility bounds of deep_table_index, the path's own (tests lower LAYER2_* / LAYER3_* on small blocks and pin the launches
    # that result), all about profit only and all measured (profiles/deep_layer_tables_ab.md).  The deepest level built: on
    # COX2-shaped x64 every level up to the eighth made the pass faster than the level before it (22.03, 20.93, 19.71, 18.44,
    # 17.63, 16.74 ms for K = 3 .. 8).  The most classes of a level: the largest table measured, 37 756 rows (9.7 MB, beyond one
    # XCD's L2), costs the walk no more per row than the 3 MB one; the next power of two above it.  The fewest rows per class: as
    # the third layer's.  The fewest count rows: the path already pays at 650 110 rows (neighborhood model 1.331 -> 1.218 ms), the
    # smallest block that has the third layer's table at its default bounds; the tests that pin the launches of a 525 460-row
    # block at the default bounds want at least 2^20
    DEEP_TABLE_MAX_LEVEL = 8
    DEEP_TABLE_MAX_CLASSES = 1 << 16
    DEEP_TABLE_MIN_ROWS_PER_CLASS = 8
    DEEP_TABLE_MIN_ROWS = 1 << 20

    def deep_table_index(self):
        """The count rows' classes under the layers BEYOND the third (built once per batch, on the batch's device): a list with
        one tuple ``(cls_k, rep_uptr, rep_vcol, rep_self, vcol_k, ccls_km1, crep_km1)`` per level k = 4, 5, ..., each laid out
        as ``layer3_table_index`` lays out k = 3; empty where ``layer3_table_index`` is None.

        The recurrence is the third layer's: a canonical row of X_{k-1} is a function of its own canonical class of X_{k-2} and,
        per CSR entry in order, of the source's count class of X_{k-2} (``ccls_km1`` [B], ``crep_km1`` the lowest canonical row of
        each class); a count row of X_k is a function of its own class of X_{k-1} and, per entry, of the source's class of
        X_{k-1} -- the count class in slots 0 and 1, the canonical class in the table slots.  ``rep_uptr`` / ``rep_vcol`` are the
        compact CSR of the lowest row of each class with the sources so remapped (rows of table_{k-1}; rows of the table product
        on the ``crep_km1`` rows), ``rep_self`` the representatives' own rows in table_{k-1}, ``vcol_k`` = ``vcol`` with the
        sources of slots 0 and 1 replaced by ``cls_k``.  Exact (``_refine_classes``).  The list stops before the first level
        with more than DEEP_TABLE_MAX_CLASSES classes or fewer than DEEP_TABLE_MIN_ROWS_PER_CLASS rows per class, and at
        DEEP_TABLE_MAX_LEVEL; blocks of fewer than DEEP_TABLE_MIN_ROWS count rows build nothing."""
        if "_deep_table" in self.__dict__:
            return self.__dict__["_deep_table"]
        self.__dict__["_deep_table"] = res = self._build_deep_tables()
        for k, level in enumerate(res, 4):
            self._check_level_ids(level, self._table_level(k - 1)[3].numel())
        return res

    def _build_deep_tables(self):
        nc = self.num_count
        levels = []
        if nc < self.DEEP_TABLE_MIN_ROWS or self.DEEP_TABLE_MAX_LEVEL < 4:      # (small blocks leave before any work)
            return levels
        prev = self.layer3_table_index()
        if prev is None:
            return levels
        before, c = self.layer2_table_index(), self._level_csr()
        umax = min(self.DEEP_TABLE_MAX_CLASSES, nc // self.DEEP_TABLE_MIN_ROWS_PER_CLASS)
        size = lambda level: (level[1].numel() - 1) // self.slots
        for k in range(4, self.DEEP_TABLE_MAX_LEVEL + 1):
            # level k from level k - 1 (``prev``: its count classes, the canonical classes it was built on) and the count classes
            # of level k - 2 (``before``), which with those canonical classes are what the entries' sources were at level k - 1
            key, ckey, uc = prev[0].to(torch.int64), prev[5].to(torch.int64), prev[6].numel()
            ent = torch.where(c.low, before[0].to(torch.int64)[c.csrc], ckey[c.qsrc])
            r = self._next_level(c, key, size(prev), ckey, uc, ent, max(size(before), uc), umax)
            if r is None:
                break
            levels.append(r)
            before, prev = prev, r
        return levels

    # eligibility bounds of anchor_class_index, the path's own and about profit only (tests lower the bounds above on small
    # blocks and pin the launches that result; this index stays off there).  Both apply to the NEIGHBORHOODS, one canonical row
    # each: what the table form saves -- the anchor MLP on all but U_a rows -- grows with them, what it adds (a gather of U_a
    # rows, a U_a-row GEMM launch) does not
    ANCHOR_CLASS_MIN_ROWS = 1 << 20
    ANCHOR_CLASS_MIN_ROWS_PER_CLASS = 8

    def anchor_class_index(self, layer_num: int):
        """The canonical rows' classes under the LAST layer of a model of ``layer_num`` = L layers (built once per batch and L,
        on the batch's device): ``(acls, arep)`` or None.  The recurrence of ``deep_table_index`` one step on: a canonical row
        of X_L is a function of its own canonical class of X_{L-1} (the deepest level's ``ccls``) and, per CSR entry in order,
        of the source's count class of X_{L-1}.  The classes of each level refine those of the level before, so rows of one
        class agree in their canonical rows of EVERY layer -- in the whole anchor operand [X_1 | ... | X_L] and in its row
        bound: ``acls`` [B] int32 is each neighborhood's class, ``arep`` [U_a] int64 the lowest canonical row of each class
        (an index into the B canonical rows).  Exact (``_refine_classes``).  None unless the table levels reach the model's
        last layer (``len(deep_table_index()) == L - 3``), the block has at least ANCHOR_CLASS_MIN_ROWS neighborhoods and
        ANCHOR_CLASS_MIN_ROWS_PER_CLASS U_a <= B."""
        cache = self.__dict__.setdefault("_anchor_class", {})
        if layer_num not in cache:
            cache[layer_num] = res = self._build_anchor_classes(layer_num)
            if res is not None and res[0].is_cuda:
                from . import ops
                # the classes address the table of the distinct anchor rows (desco_pool_post_rows_bf16x6_f32)
                ops.index_range_check(res[0], res[1].numel())
        return cache[layer_num]

    def _build_anchor_classes(self, L):
        B = self.num_rows - self.num_count
        if L < 4 or B < self.ANCHOR_CLASS_MIN_ROWS:                             # (small blocks leave before any work)
            return None
        deep = self.deep_table_index()
        if len(deep) != L - 3:
            return None
        top, below, c = deep[-1], self._table_level(L - 1), self._level_csr()
        key, u = below[0].to(torch.int64), (below[1].numel() - 1) // self.slots    # count classes of X_{L-1}
        ckey, uc = top[5].to(torch.int64), top[6].numel()                          # canonical classes of X_{L-1}
        ent = torch.where(c.low, key[c.csrc], ckey[c.qsrc])
        r = self._refine_classes(ckey, uc, c.cstart, c.ctdeg, ent, c.cdmax, max(u, uc) + 1,
                                 B // self.ANCHOR_CLASS_MIN_ROWS_PER_CLASS)
        if r is None:
            return None
        acls, ua = r
        return (acls.to(torch.int32).contiguous(), self._lowest_rows(acls, ua).contiguous())

    # eligibility bounds of pool_class_index, the path's own and about profit only, on the NEIGHBORHOODS like the anchor
    # index's: what the class form saves -- the pooling walk, post_mp.0, the tail and the count head on all but U_p rows --
    # grows with them, what it adds (a U_p-row launch of each, a gather of [B, Q] counts) does not.  Tests on small blocks lower
    # them on their batch object; at the defaults those blocks keep the launches their tests pin
    POOL_CLASS_MIN_ROWS = 1 << 20
    POOL_CLASS_MIN_ROWS_PER_CLASS = 8

    def pool_class_index(self, layer_num: int):
        """The neighborhoods' classes under everything behind the trunk of a model of ``layer_num`` = L layers (built once per
        batch and L, on the batch's device): ``(pcls, prep)`` or None; defined only where ``anchor_class_index(L)`` is.

        post_mp.0's operand row of neighborhood b is its anchor row plus, per layer, the pooled sum of its count rows as the
        fused pooling forms it: running sums in row order, cut at the 16-row tile boundaries of the GLOBAL row index, the
        pieces added left to right.  Every summand is a row of a class table and the classes nest, so the whole row is a
        function of the anchor class ``acls[b]``, of ``count_ptr[b] & 15`` (where the cuts fall inside the neighborhood) and
        of the ordered top-level count classes of its rows; all that follows -- post_mp, the count head -- is row-local.
        ``pcls`` [B] int32 is each neighborhood's class under that triple, ``prep`` [U_p] int64 the lowest neighborhood of
        each class.  Exact (``_refine_classes``).  None unless the block has at least POOL_CLASS_MIN_ROWS neighborhoods and
        POOL_CLASS_MIN_ROWS_PER_CLASS U_p <= B."""
        cache = self.__dict__.setdefault("_pool_class", {})
        if layer_num not in cache:
            cache[layer_num] = res = self._build_pool_classes(layer_num)
            if res is not None and res[0].is_cuda:
                from . import ops
                # the classes address the representatives' rows of counts (desco_gather_rows_f32)
                ops.index_range_check(res[0], res[1].numel())
        return cache[layer_num]

    def _build_pool_classes(self, L):
        B = self.num_rows - self.num_count
        if B < max(self.POOL_CLASS_MIN_ROWS, 1):                                # (small blocks leave before any work)
            return None
        ac = self.anchor_class_index(L)
        if ac is None:
            return None
        top = self._table_level(L)                                              # (there: the anchor index needs level L)
        cls, u = top[0].to(torch.int64), (top[1].numel() - 1) // self.slots
        cp = self.count_ptr.to(torch.int64)
        start, rows = cp[:-1], cp[1:] - cp[:-1]
        # the start key, made dense: the anchor class and the neighborhood's first row inside its tile
        uniq, key = torch.unique(ac[0].to(torch.int64) * 16 + (start & 15), return_inverse=True)
        r = self._refine_classes(key, uniq.numel(), start, rows, cls, int(rows.max().item()), u + 1,
                                 B // self.POOL_CLASS_MIN_ROWS_PER_CLASS)
        if r is None:
            return None
        pcls, up = r
        return (pcls.to(torch.int32).contiguous(), self._lowest_rows(pcls, up).contiguous())

    def pool_class_launch_index(self, layer_num: int):
        """What the pass needs to run on the representatives of ``pool_class_index(layer_num)`` (built once, on the device):
        a ``_PoolClasses`` or None.  ``rep_ptr`` [U_p + 1] int32 is the representatives' compact row pointer (their row
        counts, summed), ``bits`` / ``slot`` / ``nslots`` its fused-pooling index, ``anch_row`` [U_p] int32 their anchor
        classes."""
        cache = self.__dict__.setdefault("_pool_class_launch", {})
        if layer_num not in cache:
            idx = self.pool_class_index(layer_num)
            if idx is not None:
                from . import ops
                pcls, prep = idx
                cp = self.count_ptr.to(torch.int64)
                rows = (cp[1:] - cp[:-1])[prep]
                rep_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=rows.device), rows.cumsum(0)])
                total = int(rep_ptr[-1].item())
                rep_ptr = rep_ptr.to(torch.int32).contiguous()
                bits, slot, totals = ops.pool_index_dev(rep_ptr, prep.numel(), total)
                nslots, _, smallest, _ = totals.tolist()
                if smallest <= 0:
                    raise ValueError("fused pooling needs at least one count row per neighborhood")
                idx = _PoolClasses(pcls, prep, rep_ptr, bits, slot, int(nslots),
                                   self.anchor_class_index(layer_num)[0][prep].contiguous())
            cache[layer_num] = idx
        return cache[layer_num]

    def canonical_class_tables(self, layer_num: int):
        """What the pass needs to keep the canonical rows of X_1 .. X_L as tables of their distinct rows (built once per batch
        and L = ``layer_num``, on the batch's device; gnn_model.CANON_CLASS_TABLES): a ``_CanonTables`` or None; defined only
        where ``anchor_class_index(L)`` is.  The canonical classes exist already -- level 1: ``canonical_table_index()[1]``,
        levels 2 .. L - 1: the ``ccls`` / ``crep`` of the table levels, level L: ``anchor_class_index`` -- and nest.

        ``size[l - 1]`` = U_c,l, the classes of level l = 1 .. L, and ``offset[l - 1]`` the first row of table l in ONE
        [sum U_c,l, 64] buffer of all of them.  ``uptr1`` [U_c,1 S + 1] is the row-pointer array of the distinct canonical
        degree tuples (input of desco_degree_affine_f32: table 1).  ``levels[l - 2]``, l = 2 .. L, = ``(rep_uptr, rep_vcol,
        below)``: the compact 4-slot CSR of the lowest canonical row of each class of level l, its sources -- count rows --
        remapped to their count classes of X_{l-1} (rows of the count rows' table l - 1), and ``below`` [U_c,l] int64 the
        representatives' own classes of level l - 1 (their own rows in table l - 1).  ``anchor_rows`` [U_a L] int64: per
        anchor class and level the buffer row of the representative's class of that level -- the anchor operand's blocks."""
        cache = self.__dict__.setdefault("_canon_tables", {})
        if layer_num not in cache:
            cache[layer_num] = self._build_canonical_tables(layer_num)
        return cache[layer_num]

    def _build_canonical_tables(self, L):
        ac = self.anchor_class_index(L)
        if ac is None:
            return None
        S, nc = self.slots, self.num_count
        c = self._level_csr()
        tab1, ctab = self._table_indices()
        vr = self.vrowptr.to(torch.int64)
        ne = c.col.numel()
        if ne == 0 or not bool(c.low[int(vr[S * nc]):].all()):           # (a canonical row's sources are count rows)
            return None
        cdeg = (vr[1:] - vr[:-1])[S * nc:].view(-1, S)
        # count classes of X_1 .. X_{L-1} and their number; canonical classes of X_1 .. X_L and their lowest rows
        cls, u = {1: tab1[1]}, {1: tab1[0].numel() // S}
        for k in range(2, L):
            t = self._table_level(k)
            cls[k], u[k] = t[0], (t[1].numel() - 1) // S
        ccls, crep = {1: ctab[1].to(torch.int64), L: ac[0].to(torch.int64)}, {L: ac[1]}
        for l in range(2, L):
            t = self._table_level(l + 1)
            ccls[l], crep[l] = t[5].to(torch.int64), t[6]
        size = [(ctab[0].numel() - 1) // S] + [crep[l].numel() for l in range(2, L + 1)]
        offset = [sum(size[:l]) for l in range(L)]
        pos = torch.arange(max(c.cdmax, 1), device=vr.device)
        i32 = lambda t: t.to(torch.int32).contiguous()
        levels = []
        for l in range(2, L + 1):
            rep = crep[l]
            ent = cls[l - 1].to(torch.int64)[c.csrc]
            rep_uptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=vr.device), cdeg[rep].reshape(-1).cumsum(0)])
            idx = c.cstart[rep][:, None] + pos[None, :]
            rep_vcol = i32(ent[idx.clamp(max=ne - 1)][pos[None, :] < c.ctdeg[rep][:, None]])
            below = ccls[l - 1][rep].contiguous()
            # every id that a kernel uses as an address, checked once: the sources (rows of the count table l - 1) and the
            # representatives' own rows (rows of the canonical table l - 1)
            if rep_vcol.is_cuda:
                from . import ops
                ops.index_range_check(rep_vcol, u[l - 1])
                ops.index_range_check(i32(below), size[l - 2])
            levels.append((i32(rep_uptr), rep_vcol, below))
        arep = ac[1]
        anchor_rows = torch.stack([offset[l - 1] + ccls[l][arep] for l in range(1, L + 1)], dim=1).reshape(-1).contiguous()
        if anchor_rows.is_cuda:
            from . import ops
            for l in range(1, L + 1):
                ops.index_range_check(i32(ccls[l][arep]), size[l - 1])
        return _CanonTables(ctab[0], levels, size, offset, anchor_rows)

    @property
    def table_empty(self) -> int:
        """Which of the count rows' two TABLE slots -- the canonical->count relations: CSR slot 2 (triangle, table slot 0) and
        CSR slot 3 (tride, table slot 1) -- have no entry in the whole block: bit t set = table slot t is empty.  Molecule
        graphs have no triangles (1); the count launches then need no table columns for that relation
        (gnn_model.TABLE_NARROW).  Two reductions over the count rows' pointers on the device and one read-back, cached;
        the host-prologue path reads its numpy arrays."""
        v = self.__dict__.get("_table_empty")
        if v is None:
            S, nc = self.slots, self.num_count
            if nc == 0:
                tot = (0, 0)
            elif self._pool_on_device():
                vr = self.vrowptr
                tot = torch.stack([(vr[s + 1:S * nc + 1:S] - vr[s:S * nc:S]).sum() for s in (S - 2, S - 1)]).tolist()
            else:
                vr = np.asarray(self.part.vrowptr).astype(np.int64)
                tot = [int((vr[s + 1:S * nc + 1:S] - vr[s:S * nc:S]).sum()) for s in (S - 2, S - 1)]
            v = self.__dict__["_table_empty"] = (1 if tot[0] == 0 else 0) | (2 if tot[1] == 0 else 0)
        return v

    @property
    def table1_empty(self) -> bool:
        """table slot 1 (CSR slot 3) has no entry in the block"""
        return bool(self.table_empty & 2)

    # PyG-style views -----------------------------------------------------------------------
    @property
    def node_feature_dict(self) -> Dict[str, torch.Tensor]:
        f = self.node_feature
        if f is None:
            f = torch.zeros((self.num_rows, self.input_dim), device=self.device)
        return {"count": f[:self.num_count], "canonical": f[self.num_count:]}

    @property
    def edge_index_dict(self):
        return {k: torch.from_numpy(v) for k, v in self.part.edge_index_dict().items()}

    @property
    def batch_dict(self):
        b = np.repeat(np.arange(self.num_graphs), np.diff(self.part.count_ptr))
        return {"count": torch.from_numpy(b), "canonical": torch.arange(self.num_graphs)}


def tconv_split(n: int, edges) -> Tuple[np.ndarray, np.ndarray]:
    """Directed edges (src, dst) of an undirected graph and their tride flag.

    tride = NOT(endpoints share a neighbour) -- ToTconvHetero, transforms.py:201-221
    (T = A*(A@A) + A, triangle iff T > 1)."""
    A = np.zeros((n, n), dtype=np.int64)
    for a, b in edges:
        if a != b:
            A[a, b] = A[b, a] = 1
    T = A * (A @ A) + A
    src, dst = np.nonzero(A)
    return np.stack([src, dst]), T[src, dst] <= 1


class QueryBatch(_TrainIndexMixin):
    """The query graphs as one single-type ("union_node") block with 2 relation slots
    (union_triangle, union_tride) -- lightning_model.py:37-87, 291-309."""

    slots = 2

    def __init__(self, queries: Sequence[Tuple[int, Sequence[Tuple[int, int]]]], device,
                 input_dim: int = 1, node_feature: Optional[torch.Tensor] = None):
        """``node_feature`` [sum of query sizes, input_dim]: the labelled queries of --use_node_feature
        (one-hot rows, main.py:51-62); None = zeros (the unlabelled standard queries)."""
        self.queries = [(int(n), [tuple(e) for e in es]) for n, es in queries]
        self.device = _norm_device(device)
        device = self.device
        self.input_dim = input_dim
        sizes = np.array([n for n, _ in self.queries], dtype=np.int64)
        gp = np.concatenate([[0], np.cumsum(sizes)])
        N = int(gp[-1])
        cnt = np.zeros(2 * N, dtype=np.int64)
        ents = []
        for g, (n, es) in enumerate(self.queries):
            ei, tride = tconv_split(n, es)
            for (s, d), t in zip(ei.T.tolist(), tride.tolist()):
                ents.append(((d + gp[g]) * 2 + int(t), s + gp[g]))
        ents.sort()
        for v, _ in ents:
            cnt[v] += 1
        self.num_graphs = len(self.queries)
        self.num_rows = N
        self.graph_ptr_host = gp
        self.vrowptr = _i32(np.concatenate([[0], np.cumsum(cnt)]), device)
        self.vcol = _i32(np.array([c for _, c in ents], dtype=np.int64), device)
        self.graph_ptr = _i32(gp, device)
        self.node_feature = None
        if node_feature is not None:
            nf = torch.as_tensor(node_feature, dtype=torch.float32)
            if nf.shape != (N, input_dim):
                raise ValueError(f"query node_feature must be [{N}, {input_dim}], got {tuple(nf.shape)}")
            self.node_feature = nf.to(device).contiguous()

    def _seg_ptr_host(self):
        return self.graph_ptr_host

    def _seg_ptr_device(self):
        return self.graph_ptr


def _graphset_device_csr(graphs: GraphSet, device: torch.device):
    """(rowptr int64, col int32) of a GraphSet on ``device``, uploaded once per set and device: every GraphBatch over
    a graph range of the set reads the same two tensors."""
    cache = graphs.__dict__.setdefault("_device_csr", {})
    if device not in cache:
        cache[device] = (torch.from_numpy(graphs.rowptr).to(device), torch.from_numpy(graphs.col).to(device))
    return cache[device]


class GraphBatch(_TrainIndexMixin):
    """Whole target graphs as one single-type ("union_node") block with 2 relation slots (union_triangle, union_tride):
    the whole-graph twin of ``QueryBatch`` -- the same arrays -- for the model without canonical partition
    (NeighborhoodCountingModel.to_hetero_wo_canonical; reference workload.py:800-833).  Graphs [g0, g1) of a
    ``GraphSet``.  On a cuda device the typed CSR is built there from the set's device CSR (desco_graph_tconv_dev: the
    large arrays never visit the host); on the CPU by the host routine (desco_graph_tconv) -- in either case when
    ``vrowptr`` / ``vcol`` are first read.

    ``node_feature``: None = ZeroNodeFeat; True = the set's ``node_feat`` rows (--use_node_feature); or a
    [num_rows, input_dim] tensor.  ``y`` [G, Q]."""

    slots = 2

    def __init__(self, graphs: GraphSet, device, g0: int = 0, g1: Optional[int] = None, node_feature=None,
                 y: Optional[torch.Tensor] = None, input_dim: int = 1):
        g1 = graphs.num_graphs if g1 is None else g1
        if not 0 <= g0 <= g1 <= graphs.num_graphs:
            raise ValueError(f"GraphBatch: graph range [{g0}, {g1}) outside the set's {graphs.num_graphs} graphs")
        self.graphs, self.g0, self.g1 = graphs, g0, g1
        self.device = _norm_device(device)
        device = self.device
        n0, n1 = int(graphs.graph_ptr[g0]), int(graphs.graph_ptr[g1])
        e0, e1 = int(graphs.rowptr[n0]), int(graphs.rowptr[n1])
        self.num_graphs, self.num_rows = g1 - g0, n1 - n0
        self.graph_ptr_host = graphs.graph_ptr[g0:g1 + 1] - n0
        if 2 * self.num_rows + 1 >= 2 ** 31 or e1 - e0 >= 2 ** 31:
            raise ValueError("graph batch too large for int32 row / edge offsets; split it")
        self._nodes, self._edges = (n0, n1), (e0, e1)
        self.graph_ptr = _i32(self.graph_ptr_host, device)
        if node_feature is True:
            if graphs.node_feat is None:
                raise ValueError("node_feature=True needs a set with node features (GraphSet.node_feat)")
            node_feature = torch.from_numpy(graphs.node_feat[n0:n1])
        self.node_feature = None
        self.input_dim = input_dim
        if node_feature is not None:
            nf = torch.as_tensor(node_feature, dtype=torch.float32)
            if nf.dim() != 2 or nf.shape[0] != self.num_rows:
                raise ValueError(f"GraphBatch: node_feature must be [{self.num_rows}, F], got {tuple(nf.shape)}")
            self.node_feature = nf.to(device).contiguous()
            self.input_dim = nf.shape[1]
        self.y = None if y is None else y.to(device)

    def __getattr__(self, name):
        # vrowptr / vcol are built when first read: a batch handed out on the CPU by a dataset and moved to the GPU
        # by the trainer (``to``) never runs the host routine, and its arrays are made where they are used
        if name not in ("vrowptr", "vcol"):
            raise AttributeError(name)
        from . import ops
        (n0, n1), (e0, e1) = self._nodes, self._edges
        if self.device.type == "cuda":
            rowptr, col = _graphset_device_csr(self.graphs, self.device)
            self.vrowptr, self.vcol = ops.graph_tconv_dev(rowptr, col, n0, n1 - n0, e0, e1 - e0)
        else:
            vr, vc = ops.graph_tconv_host(self.graphs.rowptr, self.graphs.col, n0, n1 - n0)
            self.vrowptr, self.vcol = torch.from_numpy(vr), torch.from_numpy(vc)
        return self.__dict__[name]

    def to(self, device):
        if _norm_device(device) == self.device:
            return self
        return GraphBatch(self.graphs, device, self.g0, self.g1, self.node_feature, self.y, self.input_dim)

    def _seg_ptr_host(self):
        return self.graph_ptr_host

    def _seg_ptr_device(self):
        return self.graph_ptr


class GossipBatch:
    """Whole target graphs for the gossip stage: symmetric CSR (ascending cols) + x [N,Q].

    Equivalent of the PyG ``Data`` batch of GossipDataset (workload.py:48-150) after the
    per-call canonicalisation of gnn_model.py:246-248, done once."""

    def __init__(self, graphs: GraphSet, device, x: Optional[torch.Tensor] = None,
                 y: Optional[torch.Tensor] = None):
        self.graphs = graphs
        self.device = _norm_device(device)
        device = self.device
        self.num_graphs = graphs.num_graphs
        self.num_nodes = graphs.num_nodes
        if graphs.num_directed_edges >= 2 ** 31:
            raise ValueError("gossip batch too large for int32 edge offsets; split it")
        self.rowptr = _i32(graphs.rowptr, device)
        self.col = _i32(graphs.col, device)
        self.graph_ptr = _i32(graphs.graph_ptr, device)
        self.x = None if x is None else x.to(device).float().contiguous()
        self.y = None if y is None else y.to(device)
        self._tile_perm = None
        self._plans = {}
        self._long_row_share = None
        self._work_queue = None

    def gossip_plan(self, tiled: bool = True):
        """Plan of the planned fused gossip kernel (ops.gossip_plan) in the kernel's group order with (``tiled``) or
        without the tile order: a function of the CSR alone, computed on first use and kept."""
        if tiled not in self._plans:
            from . import ops
            self._plans[tiled] = ops.gossip_plan(self.rowptr, self.col, self.num_nodes,
                                                 self.tile_perm if tiled else None)
        return self._plans[tiled]

    @property
    def long_row_share(self) -> float:
        """share of the nodes with more than four neighbours (from the host CSR; what gnn_model.gossip_takes_plan
        routes the fused gossip launch by)"""
        if self._long_row_share is None:
            deg = np.diff(np.asarray(self.graphs.rowptr))
            self._long_row_share = float((deg > 4).mean()) if deg.size else 0.0
        return self._long_row_share

    @property
    def work_queue(self):
        """Two zeroed int64 words: the work-item tickets of this batch's fused gossip launches (the kernel leaves
        them zero).  One per batch object: launches of one batch are stream-ordered; batches that run concurrently
        (other streams, other graph replays) each have their own."""
        if self._work_queue is None:
            self._work_queue = torch.zeros(2, dtype=torch.int64, device=self.device)
        return self._work_queue

    @property
    def tile_perm(self):
        """Degree-balanced row order of the fused gossip kernel's neighbour-sum phase per 128-node tile
        (ops.gossip_tile_order): a function of the CSR alone, computed on first use."""
        if self._tile_perm is None and self.device.type == "cuda":
            from . import ops
            self._tile_perm = ops.gossip_tile_order(self.rowptr, self.num_nodes)
        return self._tile_perm

    def to(self, device):
        if _norm_device(device) == self.device:
            return self
        return GossipBatch(self.graphs, device, self.x, self.y)

    @property
    def edge_index(self):
        rp = self.graphs.rowptr
        dst = np.repeat(np.arange(self.num_nodes, dtype=np.int64), np.diff(rp))
        return torch.from_numpy(np.stack([self.graphs.col.astype(np.int64), dst]))

    @property
    def batch(self):
        return torch.from_numpy(self.graphs.node_graph_ids())
