"""The two occurrence-listing entry points are declared, exported and in the ctypes signatures; the ABI version stays 6
(an addition)."""
import os
import re

from desco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("desco_list_occurrences", "desco_list_occurrences_dev")


def test_symbols_are_declared_exported_and_typed():
    src = open(os.path.join(ROOT, "include", "desco_hip.h")).read()
    assert "OCCURRENCE LISTING" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
        decl = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: argument count differs from the header"
    assert L.desco_abi_version() == _lib.ABI_VERSION == 6


def test_device_entry_point_refuses_on_the_host_side():
    """Every refusal below happens before any HIP call (the pointers are fake and never dereferenced)."""
    import numpy as np
    from desco_amd.groundtruth import match_plan
    L = _lib.lib()
    plan = match_plan([(3, [(0, 1), (1, 2)])])
    two = match_plan([(3, [(0, 1), (1, 2)]), (2, [(0, 1)])])
    p = np.zeros(64, np.int64).ctypes.data

    def call(plan_host=plan, num_queries=1, induced=1, e0=0, e1=4, E=8, cap=4, **null):
        a = {n: p for n in ("graph_ptr", "rowptr", "col", "node_graph", "bit_off", "bits", "plan_dev", "ptr", "cursor",
                            "rows", "overflow")}
        a.update(null)
        return L.desco_list_occurrences_dev(a["graph_ptr"], 1, 4, a["rowptr"], E, a["col"], a["node_graph"], a["bit_off"],
                                            a["bits"], 1, plan_host.ctypes.data if plan_host is not None else None,
                                            a["plan_dev"], len(plan_host) if plan_host is not None else 0, num_queries,
                                            induced, e0, e1, a["ptr"], 0, a["cursor"], cap, a["rows"], a["overflow"], None)

    def refused(rc, what):
        assert rc == -1
        msg = L.desco_last_error().decode()
        assert "desco_list_occurrences_dev" in msg and what in msg, msg

    refused(call(plan_host=two, num_queries=2), "plan[0] must be 1")
    refused(call(plan_host=two), "plan[0] must be 1")
    refused(call(plan_host=None), "plan[0] must be 1")
    refused(call(induced=3), "induced must be 0 or 1")
    for n in ("graph_ptr", "rowptr", "col", "node_graph", "bit_off", "bits", "plan_dev", "ptr", "cursor", "rows",
              "overflow"):
        refused(call(**{n: None}), "null pointer")
    refused(call(E=-1), "negative size")
    refused(call(cap=-1), "negative size")
    refused(call(e0=-1), "entry range")
    refused(call(e0=5, e1=4), "entry range")
    refused(call(e1=9), "entry range")
    bad = plan.copy()
    bad[2 + 4 + 2] = 7                                           # a position on a node the query does not have
    refused(call(plan_host=bad), "permute")
