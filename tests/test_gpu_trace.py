"""The receipt trace (GOSSIP_FLAG_RECEIPT_TRACE: per-peer delivery rounds and
death rounds kept on the device, gossip_trace.hip) against the CPU oracle
stepped round by round (tests/trace_ref.py) -- exact, on every path that can
produce a round's receipts.  Every case also checks the per-round stats
against the oracle's, so the flag perturbs nothing."""
import calendar
import dataclasses
import re
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

import trace_ref
from gossip_hip import Engine, Group, _abi
from gossip_hip._abi import GossipError
from gossip_hip.workloads import config

pytestmark = pytest.mark.gpu
NEVER = _abi.GOSSIP_NEVER


def _schedule(e, w):
    e.inject(w.origins, w.inject_rounds)
    if w.kills:
        e.schedule_kills([k[0] for k in w.kills], [k[1] for k in w.kills])


def _check_trace(e, ref):
    got = e.receipt_rounds()
    assert got.dtype == np.uint16 and got.shape == ref["receipt"].shape
    assert np.array_equal(got, ref["receipt"])
    assert np.array_equal(e.death_rounds(), ref["death"])
    if hasattr(e, "receipt_histogram"):
        hist = e.receipt_histogram()
        assert hist.shape == ref["hist"].shape
        assert np.array_equal(hist, ref["hist"])
        assert np.array_equal(hist, trace_ref.histogram(got, ref["rounds"]))  # a bincount of the read trace


def _run_and_check(e, w, ref, build=True):
    if build:
        e.build_graph()
    _schedule(e, w)
    e.reset()
    stats = e.run()
    assert stats == ref["stats"]
    _check_trace(e, ref)
    return stats


PATHS = [
    ("c1_ref_bootstrap_M80_kill", 1, None, {}),
    ("c2_64k_auto", 2, 1 << 16, {}),
    ("c3_256k_auto", 3, 1 << 18, {}),
    ("c3_256k_push", 3, 1 << 18, {"mode": "push"}),
    ("c3_256k_pull", 3, 1 << 18, {"mode": "pull"}),
    ("c3_256k_bin", 3, 1 << 18, {"mode": "bin"}),
    ("c3_256k_blocked", 3, 1 << 18, {"blocked": "force"}),
    ("c5_50000_churn", 5, 50_000, {}),
]


@pytest.mark.parametrize("name,idx,n,kw", PATHS, ids=[p[0] for p in PATHS])
def test_trace_on_every_path(oracle, name, idx, n, kw):
    w = config(idx, n, pick=oracle.pick_origins)
    ref = trace_ref.trace_workload(oracle, w)
    with Engine(w.n, w.n_msgs, receipt_trace=True, **w.engine_kwargs(), **kw) as e:
        _run_and_check(e, w, ref)
    if w.kills:
        for peer, rnd in w.kills:
            assert ref["death"][peer] == rnd


def test_trace_with_rebootstrap(oracle):
    w = config(5, 1 << 14, pick=oracle.pick_origins, rebootstrap=4)
    ref = trace_ref.trace_workload(oracle, w)
    with Engine(w.n, w.n_msgs, receipt_trace=True, **w.engine_kwargs()) as e:
        _run_and_check(e, w, ref)


@pytest.mark.parametrize("shape", [0, 1])
def test_trace_multiword_messages(oracle, shape):
    """The test_multiword_messages shape at M = 130 (three words, a row of 260 bytes), with churn; both store
    shapes of the trace kernel ("trace_shape")."""
    n, M = 1 << 14, 130
    rng = np.random.default_rng(M)
    origins = rng.integers(0, n, M).astype(np.uint32)
    rounds = rng.integers(0, 4, M).astype(np.uint32)
    rp, col = oracle.gen("powerlaw", n, 6, 77)
    churn = 42949673 * 2
    key = ("multiword", M)
    if key not in trace_ref._cache:
        trace_ref._cache[key] = trace_ref.trace_sim(oracle, rp, col, n, M, origins, rounds, seed=77,
                                                    churn_threshold=churn, ping_every=2, max_missed=2)
    ref = trace_ref._cache[key]
    with Engine(n, M, rng_seed=77, churn_threshold=churn, ping_every=2, max_missed=2, receipt_trace=True,
                tuning={"trace_shape": shape}) as e:
        e.load_csr(rp, col)
        e.inject(origins, rounds)
        e.reset()
        assert e.run() == ref["stats"]
        _check_trace(e, ref)


@pytest.mark.parametrize("min_rounds,lds", [(24, True), (26, False)])
def test_trace_histogram_bin_paths(oracle, min_rounds, lds):
    """k_trace_hist keeps its bins in LDS while rounds x M <= 12,288 and uses global atomics above: M = 511
    (eight words, the last one short) at 24 and 26 rounds sits on either side, and 4,099 x 511 entries are no
    multiple of the eight entries a thread loads at once."""
    n, M = 4099, 511
    rng = np.random.default_rng(M)
    origins = rng.integers(0, n, M).astype(np.uint32)
    rounds = rng.integers(0, 4, M).astype(np.uint32)
    rp, col = oracle.gen("powerlaw", n, 6, 511)
    ref = trace_ref.trace_sim(oracle, rp, col, n, M, origins, rounds, seed=511, min_rounds=min_rounds)
    assert ref["rounds"] == min_rounds and (ref["rounds"] * M <= 12288) == lds and (n * M) % 8
    with Engine(n, M, rng_seed=511, min_rounds=min_rounds, receipt_trace=True) as e:
        e.load_csr(rp, col)
        e.inject(origins, rounds)
        e.reset()
        assert e.run() == ref["stats"]
        _check_trace(e, ref)
        assert int(e.receipt_histogram().sum()) == int((ref["receipt"] != NEVER).sum())
        assert e.receipt_histogram(max_rounds=3).shape == (3, M)  # a shorter buffer: the first rounds only
        assert np.array_equal(e.receipt_histogram(max_rounds=3), ref["hist"][:3])


def test_trace_shapes_agree(oracle):
    """Both store shapes on the widest case (2^18 peers x 64 messages)."""
    w = config(3, 1 << 18, pick=oracle.pick_origins)
    ref = trace_ref.trace_workload(oracle, w)
    with Engine(w.n, w.n_msgs, receipt_trace=True, tuning={"trace_shape": 1}, **w.engine_kwargs()) as e:
        _run_and_check(e, w, ref)


def test_trace_deferred_rounds_and_mid_run_reads(oracle):
    """config 3 at 2^18 with blocked rounds off and defer_permille 10: round 2 defers its seen update and
    round 3 folds it (test_deferred_round_fold).  Driven with step(): after each of rounds 2 to 6 the trace is
    the whole run's cut at that round -- also right after the deferred round, whose receipts are not in seen."""
    w = config(3, 1 << 18, pick=oracle.pick_origins)
    ref = trace_ref.trace_workload(oracle, w)
    assert ref["rounds"] > 7
    with Engine(w.n, w.n_msgs, receipt_trace=True, blocked="off", tuning={"defer_permille": 10},
                **w.engine_kwargs()) as e:
        e.enable_timing(True)
        e.build_graph()
        _schedule(e, w)
        e.reset()
        got = []
        while True:
            st, fin = e.step()
            got.append(st)
            if 3 <= len(got) <= 7:  # after rounds 2..6
                _check_trace(e, trace_ref.cut(ref, len(got)))
            if fin:
                break
        assert got == ref["stats"]
        _check_trace(e, ref)
        assert e.kernel_time("trace")[1] == len(got)  # one launch per round
        assert e.kernel_bytes("trace") > 0 and e.kernel_time("trace_hist")[1] > 0


@pytest.mark.parametrize("tuning", [{}, {"list_cap": 64}], ids=["default", "cap_small"])
@pytest.mark.parametrize("idx", [2, 3])
def test_trace_needy_list_rounds(oracle, idx, tuning):
    w = config(idx, 1 << 18, pick=oracle.pick_origins)
    ref = trace_ref.trace_workload(oracle, w)
    with Engine(w.n, w.n_msgs, receipt_trace=True, tuning=tuning, **w.engine_kwargs()) as e:
        e.enable_timing(True)
        e.build_graph()
        _schedule(e, w)
        e.reset()
        got = []
        while True:
            st, fin = e.step()
            got.append(st)
            if fin:
                break
        assert got == ref["stats"]
        _check_trace(e, ref)
        if not tuning:
            assert e.kernel_time("pull_list")[1] > 0  # the list rounds ran


def test_trace_replay(oracle):
    w = config(3, 1 << 18, pick=oracle.pick_origins)
    ref = trace_ref.trace_workload(oracle, w)
    with Engine(w.n, w.n_msgs, receipt_trace=True, **w.engine_kwargs()) as e:
        first = _run_and_check(e, w, ref)
        assert e.kernel_bytes("#replayed_runs") == 0
        e.reset()
        assert (e.receipt_rounds() == NEVER).all()
        assert (e.death_rounds() == NEVER).all()
        assert e.receipt_histogram().shape[0] == 0
        assert e.run() == first
        assert e.kernel_bytes("#replayed_runs") == 1
        _check_trace(e, ref)


@pytest.mark.parametrize("tiny", [1, 0])
@pytest.mark.parametrize("idx,n", [(1, None), (2, 4096)])
def test_trace_small_overlays(oracle, idx, n, tiny):
    """Under the flag the one-launch run steps aside for the round-by-round engine: the results are equal."""
    w = config(idx, n, pick=oracle.pick_origins)
    ref = trace_ref.trace_workload(oracle, w)
    with Engine(w.n, w.n_msgs, receipt_trace=True, tuning={"tiny": tiny}, **w.engine_kwargs()) as e:
        _run_and_check(e, w, ref)
        e.reset()
        assert e.run() == ref["stats"]
        _check_trace(e, ref)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("idx,n", [(3, 100_003), (5, 1 << 15), (2, 40_000)])
def test_trace_group_on_one_device(oracle, idx, n, P):
    w = config(idx, n, pick=oracle.pick_origins)
    ref = trace_ref.trace_workload(oracle, w)
    with Group(w.n, w.n_msgs, [0] * P, receipt_trace=True, **w.engine_kwargs()) as g:
        g.build_graph()
        _schedule(g, w)
        g.reset()
        assert g.run() == ref["stats"]
        _check_trace(g, ref)
        # a window of 1,000 peers that straddles the first block boundary
        b = g.shape(0)["n_local"]
        lo = b - 500
        assert np.array_equal(g.receipt_rounds(lo, 1000), ref["receipt"][lo:lo + 1000])
        assert np.array_equal(g.death_rounds(lo, 1000), ref["death"][lo:lo + 1000])
        with pytest.raises(GossipError) as ei:
            g.receipt_rounds(w.n - 10, 11)
        assert ei.value.status == _abi.GOSSIP_EINVAL
        # each part's histogram over its own peers sums to the whole
        hist = np.zeros_like(ref["hist"])
        for p in range(P):
            buf = np.zeros((4096, w.n_msgs), dtype=np.uint64)
            r = _abi.C.c_uint32()
            _abi.check(_abi.lib().gossip_read_receipt_histogram(
                g.part_ctx(p), buf.ctypes.data_as(_abi.C.POINTER(_abi.C.c_uint64)), 4096, _abi.C.byref(r)), "hist")
            assert r.value == ref["rounds"]
            hist += buf[:r.value]
        assert np.array_equal(hist, ref["hist"])


def test_trace_errors():
    with Engine(4096, 8) as e:  # without the flag
        for call in (e.receipt_rounds, e.death_rounds, e.receipt_histogram):
            with pytest.raises(GossipError) as ei:
                call()
            assert ei.value.status == _abi.GOSSIP_ESTATE
            assert "GOSSIP_FLAG_RECEIPT_TRACE" in str(ei.value)
    with Group(4096, 8, [0, 0]) as g:
        for call in (g.receipt_rounds, g.death_rounds):
            with pytest.raises(GossipError) as ei:
                call()
            assert ei.value.status == _abi.GOSSIP_ESTATE
    with Engine(4096, 8, receipt_trace=True) as e:
        assert e.receipt_rounds(4095, 1).shape == (1, 8)
        assert e.receipt_rounds(4096, 0).shape == (0, 8)
        for call in (e.receipt_rounds, e.death_rounds):
            for first, count in ((4095, 2), (4097, 0), (0, 4097)):
                with pytest.raises(GossipError) as ei:
                    call(first, count)
                assert ei.value.status == _abi.GOSSIP_EINVAL
    for bad in ({"rejoin_threshold": 1000}, {"max_rounds": 70000}):
        with pytest.raises(GossipError) as ei:
            Engine(4096, 8, receipt_trace=True, **bad)
        assert ei.value.status == _abi.GOSSIP_EINVAL
        assert "GOSSIP_FLAG_RECEIPT_TRACE" in str(ei.value)
    with Engine(4096, 8, receipt_trace=True, max_rounds=65535):
        pass


# ---- the drop-in surface: network.txt trace=1 (driven as test_gpu_surface.py drives the CLI) ----
REPO = Path(__file__).resolve().parent.parent
EXE = REPO / "p2p-gossipprotocol_amd" / "build" / "gossip_peer_network"
EPOCH = 1740441600  # the simulation clock's round 0 (include/gossip/formats.hpp)
_ENTRY = re.compile(r"^(\w{3} \w{3} [ \d]\d \d\d:\d\d:\d\d \d{4})\n: (Generated message|Received new message): (.*)$", re.M)


def _cli(tmp_path, name, keys):
    cfg = tmp_path / f"{name}.txt"
    cfg.write_text((REPO / "tests" / "golden" / "network.txt").read_text() + keys)
    logs = tmp_path / name
    logs.mkdir()
    r = subprocess.run([str(EXE), str(cfg), "--logs", str(logs)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return logs, r.stdout


def _surface_workload(oracle, n, kills):
    """What network.txt's defaults make of n_peers=n graph=powerlaw origins=4: 10 messages per origin, one
    every 5 rounds, a ping round every 15, 3 missed pings."""
    w = config(2, n, pick=oracle.pick_origins)
    o = oracle.pick_origins(n, 0x5EED0001, 4)
    return dataclasses.replace(w, name=f"surface_{n}", n_msgs=40, origins=np.repeat(o, 10).astype(np.uint32),
                               inject_rounds=np.tile(np.arange(10, dtype=np.uint32) * 5, 4), rng_seed=0x5EED0001,
                               kills=kills, ping_every=15, max_missed=3)


def test_surface_logs_identical_with_and_without_the_device_trace(tmp_path):
    keys = "n_peers=3000\ngraph=powerlaw\norigins=4\nkills=5@3\n"
    plain, out0 = _cli(tmp_path, "plain", keys)
    traced, out1 = _cli(tmp_path, "traced", keys + "trace=1\n")
    rounds = [l for l in out0.splitlines() if l.startswith('{"round"')]
    assert rounds and rounds == [l for l in out1.splitlines() if l.startswith('{"round"')]
    names = sorted(p.name for p in plain.iterdir())
    assert len([x for x in names if x.startswith("peer_")]) == 3000
    assert names == sorted(p.name for p in traced.iterdir())
    for name in names:
        assert (plain / name).read_bytes() == (traced / name).read_bytes(), name


def test_surface_logs_above_the_host_capture_limit(oracle, tmp_path):
    """6,000 peers (> kTraceMax): without trace=1 no peer log is written; with it every peer's log is, and the
    "Generated message" / "Received new message" entries of peers 0, 2999 and 5999 sit at the oracle's rounds,
    in order."""
    keys = "n_peers=6000\ngraph=powerlaw\norigins=4\nkills=5@3\n"
    plain, _ = _cli(tmp_path, "plain", keys)
    assert not [p for p in plain.iterdir() if p.name.startswith("peer_")]
    traced, out = _cli(tmp_path, "traced", keys + "trace=1\n")
    assert len([p for p in traced.iterdir() if p.name.startswith("peer_")]) == 6000
    w = _surface_workload(oracle, 6000, [(5, 3)])
    ref = trace_ref.trace_workload(oracle, w)
    rounds = [l for l in out.splitlines() if l.startswith('{"round"')]
    assert len(rounds) == ref["rounds"]
    for v in (0, 2999, 5999):
        text = (traced / f"peer_{5000 + v}_output.txt").read_text()
        got = [(calendar.timegm(time.strptime(t, "%a %b %d %H:%M:%S %Y")) - EPOCH, kind, body)
               for t, kind, body in _ENTRY.findall(text)]
        want = []
        for r, m in sorted((int(ref["receipt"][v, m]), m) for m in range(w.n_msgs) if ref["receipt"][v, m] != NEVER):
            own = int(w.origins[m]) == v and int(w.inject_rounds[m]) == r
            want.append((r, "Generated message" if own else "Received new message",
                         f"Message from 127.0.0.1:{5000 + int(w.origins[m])}"))
        assert want and got == want, v
    # peer 5 died in round 3: its neighbours report it after 3 missed pings and log the disconnect
    assert ref["death"][5] == 3
    assert sum("Peer disconnected: 127.0.0.1:5005" in p.read_text() for p in traced.iterdir()
               if p.name.startswith("peer_")) > 0


@pytest.mark.parametrize("n_gpus", [1, 2])
def test_surface_receipt_round_at_any_size(oracle, tmp_path, n_gpus):
    """GossipNetwork::receiptRound with trace=1 on 70,000 peers (above every host-side limit: one peer's row is
    fetched per query), as one partition and as a group of two: the oracle's rounds, -1 for never."""
    import ctypes as C
    n = 70_000
    w = _surface_workload(oracle, n, [(5, 3)])
    ref = trace_ref.trace_workload(oracle, w)
    cfg = tmp_path / "network.txt"
    cfg.write_text((REPO / "tests" / "golden" / "network.txt").read_text() +
                   f"n_peers={n}\ngraph=powerlaw\norigins=4\nkills=5@3\ntrace=1\nn_gpus={n_gpus}\n")
    L = C.CDLL(str(EXE.parent / "libgossip_surface.so"))
    peers = np.array([0, 5, 4095, 4096, 34_999, 35_000, 35_071, 60_001, n - 1], dtype=np.uint64)
    out = np.zeros((peers.size, w.n_msgs), dtype=np.int32)
    M = C.c_uint()
    L.gossip_surface_receipt_rounds.argtypes = [C.c_char_p, C.POINTER(C.c_ulonglong), C.c_uint, C.POINTER(C.c_int),
                                                C.c_size_t, C.POINTER(C.c_uint)]
    rc = L.gossip_surface_receipt_rounds(str(cfg).encode(), peers.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                         peers.size, out.ctypes.data_as(C.POINTER(C.c_int)), out.size, C.byref(M))
    assert rc == 0 and M.value == w.n_msgs
    want = ref["receipt"][peers.astype(np.int64)].astype(np.int32)
    want[want == NEVER] = -1
    assert np.array_equal(out, want)
