"""CPU tests of the receipt trace's boundary: the oracle-stepping helper that
the GPU tests compare against checks itself, the header declares the trace
readers and the library exports them, and the Python constants equal the
header's."""
import re

import numpy as np
import pytest

import trace_ref
from gossip_hip import _abi
from gossip_hip.workloads import config

READERS = ("gossip_read_receipt_rounds", "gossip_read_death_rounds", "gossip_read_receipt_histogram",
           "gossip_group_read_receipt_rounds", "gossip_group_read_death_rounds")


@pytest.mark.parametrize("idx,n", [(1, 8), (2, 4096), (5, 4096)])
def test_helper_counts_equal_the_oracle_stats(oracle, idx, n):
    """A bit appears in seen only as a first receipt or an injection (step_fast,
    gossip_oracle.c:698-742), so the entries equal to r are round r's
    new_receipts + injected of the same oracle run -- and of the oracle's own
    run to the end (oracle_sim_run), which the stepped run must reproduce."""
    w = config(idx, n, pick=oracle.pick_origins)
    rp, col = oracle.gen_workload(w)
    ref = trace_ref.trace_workload(oracle, w, rp, col)
    whole = oracle.simulate_workload(w, rp, col)
    assert ref["stats"] == whole["stats"]
    counts = np.bincount(ref["receipt"].ravel(), minlength=trace_ref.NEVER + 1)
    for r, st in enumerate(ref["stats"]):
        assert counts[r] == st["new_receipts"] + st["injected"], r
    assert counts[len(ref["stats"]):trace_ref.NEVER].sum() == 0
    # the final state: a pair has a round iff its bit is in the final seen set; a peer has a death round iff dead
    assert np.array_equal(ref["receipt"] != trace_ref.NEVER, trace_ref._bits(whole["seen"], w.n_msgs))
    assert np.array_equal(ref["death"] != trace_ref.NEVER, whole["alive"] == 0)
    assert [int(x) for x in ref["hist"].sum(axis=1)] == [s["new_receipts"] + s["injected"] for s in ref["stats"]]
    for k in w.kills:
        assert ref["death"][k[0]] == k[1]


def test_cut_is_the_stopped_run(oracle):
    """The trace of a run stopped by max_rounds is the whole run's trace cut at that round."""
    w = config(5, 4096, pick=oracle.pick_origins)
    rp, col = oracle.gen_workload(w)
    ref = trace_ref.trace_workload(oracle, w, rp, col)
    stop = 4
    assert stop < ref["rounds"]
    short = trace_ref.trace_workload(oracle, w, rp, col, max_rounds=stop)
    got = trace_ref.cut(ref, stop)
    assert short["rounds"] == stop
    for key in ("receipt", "death", "hist"):
        assert np.array_equal(short[key], got[key]), key


def test_header_declares_and_library_exports_the_readers(hip_lib):
    names = _abi.declared_symbols()
    for name in READERS:
        assert name in names, name
        assert hasattr(hip_lib, name), name
        assert getattr(hip_lib, name).argtypes is not None, name


def test_constants_equal_the_header():
    text = _abi.HEADER.read_text()

    def define(name):
        m = re.search(r"^#define\s+%s\s+(0[xX][0-9a-fA-F]+|\d+)[uU]?\b" % name, text, re.M)
        assert m, name
        return int(m.group(1), 0)

    assert _abi.FLAG_RECEIPT_TRACE == define("GOSSIP_FLAG_RECEIPT_TRACE") == 256
    assert _abi.GOSSIP_NEVER == define("GOSSIP_NEVER") == 0xFFFF == trace_ref.NEVER
    # the flag is its own bit
    others = [int(v, 0) for v in re.findall(r"^#define\s+GOSSIP_FLAG_(?!RECEIPT_TRACE)\w+\s+(\d+)u", text, re.M)]
    assert others and all(v & _abi.FLAG_RECEIPT_TRACE == 0 for v in others)


def test_make_config_sets_the_flag():
    from gossip_hip.engine import make_config
    assert make_config(64, 8).flags & _abi.FLAG_RECEIPT_TRACE == 0
    assert make_config(64, 8, receipt_trace=True).flags & _abi.FLAG_RECEIPT_TRACE
