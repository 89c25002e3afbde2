"""CPU tier: Multi-Krum (FED.ROBUST_AGG multi_krum; Blanchard et al., NeurIPS 2017; El Mhamdi et al., ICML 2018) through
the collective protocol of federated_multi_modal_amd/federated.py on gloo ranks, with the host restatements of
tests/_krum_ref.py in the kernels' place (the GPU tier, tests/test_fedavg_krum_gpu.py, checks the kernels against the
same restatements).

Given the selection, the mean of the selected clients in client order depends on no layout, so every layout of a
client set must give the bits of the restatement over all its clients' buckets in one process.  The fp64 distances may
differ between layouts in their last bits (the shard boundaries move), so every such comparison first checks, with
stable_selection, that the selection does not hang on those bits."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from _krum_ref import gamma2, host_pairwise, host_select, host_selected_mean, stable_selection
from test_fedavg_compress_dist import CompressHostKernels
from test_fedavg_compress_dist import run_rounds as compress_rounds
from test_fedavg_dist import _init, _spawn
from test_fedavg_robust_dist import N, N16, RobustHostKernels, client_engine, global_engine

NAN = float("nan")


class KrumHostKernels(RobustHostKernels):
    """The host kernels plus Multi-Krum's, with the signatures of ops.krum_ws_bytes, ops.krum_pairwise,
    ops.krum_select and ops.fedavg_reduce_selected."""

    @staticmethod
    def krum_ws_bytes(nclients, n):
        return 8

    @staticmethod
    def krum_pairwise(gathered, nclients, n, ws, dist_out):
        assert dist_out.dtype == torch.float64 and dist_out.numel() == nclients * nclients
        g = gathered.view(nclients, -1)[:, :n]
        dist_out.copy_(torch.from_numpy(host_pairwise(g)).view(-1))

    @staticmethod
    def krum_select(parts, nclients, f, m, selected, scores, counts):
        sel, sc, cnt, _ = host_select(parts.view(-1, nclients, nclients).numpy(), f, m)
        selected.copy_(torch.tensor(sel, dtype=torch.int32))
        scores.copy_(torch.from_numpy(sc))
        counts.copy_(torch.tensor(cnt, dtype=torch.int32))

    @staticmethod
    def fedavg_reduce_selected(gathered, nclients, selected, count_pos, out):
        g = gathered.view(nclients, -1)[:, :out.numel()]
        out.copy_(host_selected_mean(g, selected.tolist(), count_pos))


class KrumCompressKernels(CompressHostKernels, KrumHostKernels):
    """... with the int8 codec; the selection's precondition is checked where the combined distances are at hand."""

    @staticmethod
    def krum_select(parts, nclients, f, m, selected, scores, counts):
        D = host_select(parts.view(-1, nclients, nclients).numpy(), f, m)[3]
        stable_selection(D, f, m)
        KrumHostKernels.krum_select(parts, nclients, f, m, selected, scores, counts)


# ----------------------------------------------------------------------------- the statistic itself

def _one_d(values):
    return host_pairwise(torch.tensor(values, dtype=torch.float32).view(-1, 1))


def test_worked_example():
    """The 1-D clients 0, 1, 2, 3, 100 with f = 1: scores 5, 2, 2, 5, 19013."""
    x = [0.0, 1.0, 2.0, 3.0, 100.0]
    D = _one_d(x)
    sel, scores, counts, _ = host_select(D, 1, 1)
    assert scores.tolist() == [5.0, 2.0, 2.0, 5.0, 19013.0] and counts == (5, 1, 1)
    assert sel == [0, 1, 0, 0, 0]  # the tie goes to the lower index
    g = torch.tensor(x).view(-1, 1)
    sel, _, counts, _ = host_select(D, 1, 3)
    assert sel == [1, 1, 1, 0, 0] and counts == (5, 1, 3) and host_selected_mean(g, sel).item() == 1.0
    sel, _, counts, _ = host_select(D, 1, 0)
    assert sel == [1, 1, 1, 1, 0] and counts == (5, 1, 4) and host_selected_mean(g, sel).item() == 1.5
    # a permuted client order: the same clients by value, the tie still to the lower index
    perm = [4, 2, 0, 3, 1]
    xp = [x[i] for i in perm]  # 100, 2, 0, 3, 1
    Dp = _one_d(xp)
    sel, scores, _, _ = host_select(Dp, 1, 1)
    assert scores.tolist() == [19013.0, 2.0, 5.0, 5.0, 2.0] and sel == [0, 1, 0, 0, 0]
    sel, _, _, _ = host_select(Dp, 1, 0)
    assert sel == [0, 1, 1, 1, 1] and host_selected_mean(torch.tensor(xp).view(-1, 1), sel).item() == 1.5
    # the parts are added in order, before anything is read from them
    sel2, scores2, _, D2 = host_select(np.stack([D * 0.25, D * 0.5, D * 0.25]), 1, 0)
    assert np.array_equal(D2, D) and sel2 == [1, 1, 1, 1, 0] and scores2.tolist() == [5.0, 2.0, 2.0, 5.0, 19013.0]


def test_degenerate_sizes():
    """p = 0, 1, 2, 3 present clients among 4, and an f the present ones cannot carry."""
    for present, f, m, want_sel, want_counts in (
            ((), 1, 0, [0, 0, 0, 0], (0, 0, 0)),
            ((2,), 1, 0, [0, 0, 1, 0], (1, 0, 1)),
            ((2,), 5, 3, [0, 0, 1, 0], (1, 0, 1)),
            ((0, 3), 1, 0, [1, 0, 0, 1], (2, 0, 2)),
            ((0, 3), 1, 1, [1, 0, 0, 0], (2, 0, 1)),        # q = 0: both score +0, the lower index wins
            ((0, 1, 3), 1, 0, [1, 1, 0, 1], (3, 0, 3)),     # f degrades to 0
            ((0, 1, 3), 40, 1, [1, 0, 0, 0], (3, 0, 1)),    # q = 1: clients 0 and 1 tie on their mirrored distance
    ):
        x = torch.tensor([[0.0, 0.0], [1.0, 0.0], [5.0, 5.0], [4.0, 0.0]])
        for c in range(4):
            if c not in present:
                x[c] = NAN
        D = host_pairwise(x)
        assert all(np.isnan(D[c, c]) != (c in present) for c in range(4))
        sel, scores, counts, _ = host_select(D, f, m)
        assert sel == want_sel and counts == want_counts, (present, f, m)
        assert all(np.isnan(scores[c]) != (c in present) for c in range(4))
        out = host_selected_mean(x, sel, count_pos=1)
        assert out[1].item() == float(len(present))
        assert not torch.isnan(out).any()  # an absent client's NaNs do not leak
        if not present:
            assert out[0].item() == 0.0 and not torch.signbit(out[0])
    # a large f with 8 present: f' = (8 - 3) // 2 = 2, q = 4, m' = 6
    D = _one_d([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 50.0])
    assert host_select(D, 40, 0)[2] == (8, 2, 6) and host_select(D, 40, 100)[2] == (8, 2, 6)
    assert host_select(D, 40, 0)[0] == [1, 1, 1, 1, 1, 1, 0, 0]


def test_pairwise_restatement_properties():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 1001, generator=g)
    x[4] = NAN
    x[0, 7], x[1, 7] = 3e38, -3e38  # further apart than the fp32 range: +inf, never NaN
    D = host_pairwise(x)
    assert np.array_equal(D, D.T, equal_nan=True)
    assert np.isnan(D[4]).all() and np.isnan(D[:, 4]).all() and D[0, 1] == np.inf
    assert all(D[c, c] == 0.0 and not np.signbit(D[c, c]) for c in (0, 1, 2, 3, 5))
    want = ((x[2].double() - x[3].double()) ** 2).sum().item()  # fp32 subtract against an fp64 one: close, not equal
    assert abs(D[2, 3] - want) <= 1e-6 * want
    assert 2 * 1001 * 2.0 ** -53 <= gamma2(1001) < 1e-12


# ----------------------------------------------------------------------------- every layout, one set of bits

SETTINGS = ((1, 0), (1, 1), (0, 0), (2, 3))


def scenarios(n):
    """name -> (invalid clients, finite outliers, clients that fail after they were packed)."""
    return {"clean": ((), (), ()), "bad": ((1,), (), ()), "outlier": ((), (0,), ()), "late": ((), (), (n - 1,)),
            "two": ((), (0, 2), ()), "nobody": (tuple(range(n)), (), ())}


_EXPECTED = {}


def expected(n, f, m, bad, outlier, late):
    """The single-process restatement over all n clients: (selection, n_valid, fp32 statistic or None, flat16,
    flat32), computed once per case; the selection's stability is asserted first."""
    key = (n, f, m, bad, outlier, late)
    if key not in _EXPECTED:
        rows = []
        for c in range(n):
            e = client_engine(c, bad, outlier)
            row = torch.cat([e.flat16.float(), e.flat32, torch.ones(2)])
            if c in bad or c in late:
                row = torch.full_like(row, NAN)
            rows.append(row)
        g = torch.stack(rows)
        sel = stable_selection(host_pairwise(g), f, m)
        red = host_selected_mean(g, sel, N + 1)
        p = int(red[N + 1])
        assert float(red[N]) == (1.0 if p else 0.0)  # the mean of ones is exactly 1
        if p == 0:
            ge = global_engine()
            _EXPECTED[key] = (sel, 0, None, ge.flat16, ge.flat32)
        else:
            v = (red[:N] / red[N]).half()
            _EXPECTED[key] = (sel, p, red[:N], v[:N16], v[N16:].float())
    return _EXPECTED[key]


def run_round(ids, f, m, bad, outlier, late, kernels=KrumHostKernels):
    """The clients `ids` of this process through one FedAvgExchange: pack, exchange, (late failures,) unpack."""
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    engines, feds = [], []
    for c in ids:
        e = client_engine(c, bad, outlier)
        loc16, loc32 = e.flat16.clone(), e.flat32.clone()
        e.flat16.copy_(global_engine().flat16)  # the bucket's global copy: the previous global weights
        e.flat32.copy_(global_engine().flat32)
        feds.append(FedAvgBucket(e, kernels=kernels, robust="multi_krum", krum_f=f, krum_m=m))
        e.flat16.copy_(loc16)
        e.flat32.copy_(loc32)
        engines.append(e)
    assert all(fed.buf.numel() == N + 2 for fed in feds)
    x = FedAvgExchange(feds, robust="multi_krum", krum_f=f, krum_m=m)
    for fed in feds:
        fed.pack()
    x.start()
    x.finish([j for j, c in enumerate(ids) if c in late])
    stat = feds[0].buf[:N].clone()
    stats = x.krum_stats()
    for fed in feds:
        fed.unpack()
    return x.n_valid(), stat, stats, [(e.flat16.clone(), e.flat32.clone()) for e in engines]


def _worker(rank, world, port, per_rank, out):
    _init(rank, world, port)
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    res = {}
    for f, m in SETTINGS:
        for name, (bad, outlier, late) in scenarios(world * per_rank).items():
            res[(f, m, name)] = run_round(ids, f, m, bad, outlier, late)
    out[rank] = res
    dist.destroy_process_group()


@pytest.mark.parametrize("world,per_rank", [(3, 1), (5, 1), (8, 1), (3, 2), (4, 2)])
def test_krum_exchange_is_bit_exact_at_every_layout(world, per_rank):
    """Multi-Krum at four (f, m) settings with no bad client, an invalid one, one and two finite outliers, a late
    failure and nobody valid: every rank selects what the restatement selects, the fp32 statistic and every client's
    weights equal it bit for bit, n_valid is p, and the same clients in one process give the same bits."""
    n = world * per_rank
    res = _spawn(_worker, world, per_rank)
    for f, m in SETTINGS:
        for name, (bad, outlier, late) in scenarios(n).items():
            sel, n_valid, stat, ref16, ref32 = expected(n, f, m, bad, outlier, late)
            assert n_valid == n - len(bad) - len(late)
            one = run_round(list(range(n)), f, m, bad, outlier, late)  # one process, n clients
            for got_valid, got_stat, stats, weights in [res[r][(f, m, name)] for r in range(world)] + [one]:
                where = (f, m, name)
                kept, scores, p, fe, me = stats
                assert kept == [c for c in range(n) if sel[c]], where
                assert got_valid == n_valid == p and me == sum(sel), where
                assert fe == max(min(f, (p - 3) // 2), 0), where
                assert [s != s for s in scores] == [c in bad or c in late for c in range(n)], where
                if stat is not None:
                    assert torch.equal(got_stat.view(torch.int32), stat.view(torch.int32)), where
                for p16, p32 in weights:
                    assert torch.equal(p16, ref16) and torch.equal(p32, ref32), where
            if outlier and name != "two" and f >= 1 and n >= 5:
                assert not sel[outlier[0]], (f, m, name)  # the finite outlier is dropped as a whole
            if name == "nobody":  # the round is skipped: the previous global weights
                assert n_valid == 0 and sum(sel) == 0
                assert torch.equal(ref16, global_engine().flat16) and torch.equal(ref32, global_engine().flat32)


# ----------------------------------------------------------------------------- with the int8 uplink

INT8_SCEN = (((1,), ()), ((), ()))  # round 0: client 1 invalid; round 1: everybody


def _int8_worker(rank, world, port, per_rank, out):
    _init(rank, world, port)
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    out[rank] = compress_rounds(ids, INT8_SCEN, robust="multi_krum", kernels=KrumCompressKernels)
    dist.destroy_process_group()


def test_two_int8_rounds_with_multi_krum_agree_at_every_layout():
    """Two rounds of int8 uplink compression with error feedback under Multi-Krum (f = 1, m = 0), 8 clients: 4 ranks of
    2, 8 ranks of 1 and one process end with the same weights and residuals, bit for bit (the selection's stability is
    asserted inside the host kernel, on every rank and round)."""
    one = compress_rounds(list(range(8)), INT8_SCEN, robust="multi_krum", kernels=KrumCompressKernels)
    assert one[0] == [7, 8]
    ref16, ref32, _ = one[1][0]
    assert not torch.equal(ref16, global_engine().flat16)
    for world, per_rank in ((4, 2), (8, 1)):
        res = _spawn(_int8_worker, world, per_rank)
        for r in range(world):
            valid, clients = res[r]
            assert valid == [7, 8]
            for j, (p16, p32, resid) in enumerate(clients):
                c = r * per_rank + j
                assert torch.equal(p16, ref16) and torch.equal(p32, ref32), (world, c)
                assert torch.equal(resid.view(torch.int32), one[1][c][2].view(torch.int32)), (world, c)


# ----------------------------------------------------------------------------- construction, config, ABI

def test_construction_errors():
    from federated_multi_modal_amd.federated import KRUM_TRIM, FedAvgBucket, FedAvgExchange, FedDynState, robust_trim
    e = global_engine()
    K = KrumHostKernels
    assert robust_trim("multi_krum", 1) == KRUM_TRIM and KRUM_TRIM is not None
    with pytest.raises(ValueError, match="krum"):
        FedAvgBucket(e, kernels=K, robust="krum")
    with pytest.raises(ValueError, match="multi_krum"):  # the error says what Krum is called here
        FedAvgBucket(e, kernels=K, robust="krum")
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="krum_f"):
            FedAvgBucket(e, kernels=K, robust="multi_krum", krum_f=bad)
        with pytest.raises(ValueError, match="krum_m"):
            FedAvgBucket(e, kernels=K, robust="multi_krum", krum_m=bad)
    with pytest.raises(ValueError, match="allreduce"):
        FedAvgBucket(e, kernels=K, mode="allreduce", robust="multi_krum")
    with pytest.raises(ValueError, match="weight"):
        FedAvgBucket(e, kernels=K, weight=2.0, robust="multi_krum")
    with pytest.raises(ValueError, match="topk"):
        FedAvgBucket(e, kernels=K, compress="topk", robust="multi_krum")
    with pytest.raises(ValueError, match="dyn"):
        FedAvgBucket(e, kernels=K, robust="multi_krum", dyn=FedDynState(0.1, e, 3))
    fed = FedAvgBucket(e, kernels=K, robust="multi_krum", krum_f=2, krum_m=3)
    assert fed.weighted and fed.trim == KRUM_TRIM and (fed.krum_f, fed.krum_m) == (2, 3)
    with pytest.raises(ValueError, match="krum_f"):
        FedAvgExchange([fed], robust="multi_krum", krum_f=-2, krum_m=3)
    with pytest.raises(ValueError, match="krum_m"):
        FedAvgExchange([fed], robust="multi_krum", krum_f=2, krum_m=-3)
    with pytest.raises(ValueError, match="allreduce"):
        FedAvgExchange([fed], mode="allreduce", robust="multi_krum", krum_f=2, krum_m=3)
    with pytest.raises(AssertionError):  # a bucket and an exchange that disagree
        FedAvgExchange([fed], robust="multi_krum")
    with pytest.raises(AssertionError):
        FedAvgExchange([fed], robust="median")
    clipped = FedAvgBucket(global_engine(), kernels=KrumCompressKernels, robust="multi_krum", dp_clip=1.0)
    with pytest.raises(ValueError, match="robust"):
        FedAvgExchange([clipped], robust="multi_krum", dp_std=1.0)
    x = FedAvgExchange([fed], robust="multi_krum", krum_f=2, krum_m=3)
    assert x.krum and x.selected.numel() == 1
    # the bucket alone passes its own settings on, and a single client is kept
    solo = FedAvgBucket(global_engine(), kernels=K, robust="multi_krum", krum_f=3, krum_m=1)
    assert solo.run() == 1 and solo.exchange.krum_stats()[0] == [0] and solo.exchange.krum_stats()[2:] == (1, 0, 1)
    # the other options' exchanges allocate nothing of Multi-Krum's and their host kernels (no krum attributes) serve
    from test_fedavg_dist import HostKernels
    plain = FedAvgBucket(global_engine(), kernels=HostKernels)
    assert plain.run() == 1 and plain.buf.numel() == N + 1 and not plain.exchange.krum
    med = FedAvgBucket(global_engine(), kernels=RobustHostKernels, robust="median")
    assert med.run() == 1 and not med.exchange.krum and not hasattr(med.exchange, "kpart")
    with pytest.raises(ValueError, match="multi_krum"):
        med.exchange.krum_stats()


def test_config_keys_and_trainer_validation(capsys):
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    from federated_multi_modal_amd.trainers import MaPLeFederated
    cfg = get_cfg_default()
    extend_cfg(cfg)
    assert cfg.FED.KRUM_F == 1 and cfg.FED.KRUM_M == 0 and cfg.FED.ROBUST_AGG == "none"
    cfg.merge_from_list(["FED.ROBUST_AGG", "multi_krum", "FED.KRUM_F", 2, "FED.KRUM_M", 1])
    assert cfg.FED.ROBUST_AGG == "multi_krum" and cfg.FED.KRUM_F == 2 and cfg.FED.KRUM_M == 1

    def make(num_clients=8, rank=0, **keys):
        tr = MaPLeFederated.__new__(MaPLeFederated)
        tr.num_clients, tr.rank = num_clients, rank
        fed = {"ROBUST_AGG": "multi_krum", "TRIM_K": 1, "AGGREGATION": "ordered", "CLIENT_WEIGHTS": "uniform",
               "KRUM_F": 1, "KRUM_M": 0}
        fed.update(keys)
        return tr, fed.get

    def check(**keys):
        tr, get = make(**keys)
        return tr._robust_cfg(get), tr._krum_cfg(get)

    assert check() == (("multi_krum", 1), (1, 0))
    out = capsys.readouterr().out
    assert out.count("[INFO] Robust aggregation: Multi-Krum") == 1 and "coordinate-wise" not in out
    assert check(ROBUST_AGG="Multi_Krum", KRUM_F=2, KRUM_M=6, num_clients=8) == (("multi_krum", 1), (2, 6))
    assert check(KRUM_F=0, KRUM_M=1, num_clients=3) == (("multi_krum", 1), (0, 1))
    assert "(Krum)" in capsys.readouterr().out
    check(rank=1)
    assert capsys.readouterr().out == ""  # rank 0 alone reports
    assert check(ROBUST_AGG="none", KRUM_F=30, KRUM_M=50, num_clients=2) == ((None, 1), (30, 50))  # unused, unchecked
    assert check(ROBUST_AGG="median", KRUM_F=30, num_clients=3)[0] == ("median", 1)
    for key, keys in (("FED.ROBUST_AGG", dict(ROBUST_AGG="krum")),
                      ("FED.KRUM_F", dict(KRUM_F=-1)),
                      ("FED.KRUM_F", dict(KRUM_F=1.0)),
                      ("FED.KRUM_F", dict(ROBUST_AGG="none", KRUM_F=True)),
                      ("FED.KRUM_M", dict(KRUM_M=-1)),
                      ("FED.KRUM_M", dict(KRUM_M="2")),
                      ("FED.NUM_CLIENTS", dict(KRUM_F=1, num_clients=4)),     # 2 * 1 + 3 = 5
                      ("FED.NUM_CLIENTS", dict(KRUM_F=3, num_clients=8)),     # 2 * 3 + 3 = 9
                      ("FED.NUM_CLIENTS", dict(KRUM_F=0, num_clients=2)),
                      ("FED.NUM_CLIENTS", dict(num_clients=65)),
                      ("FED.KRUM_M", dict(KRUM_M=8)),                          # at most 8 - 1
                      ("FED.AGGREGATION", dict(AGGREGATION="allreduce")),
                      ("FED.CLIENT_WEIGHTS", dict(CLIENT_WEIGHTS="samples"))):
        with pytest.raises(ValueError, match=key):
            check(**keys)
    assert check(KRUM_M=7) == (("multi_krum", 1), (1, 7))
    # the other options' validation names Multi-Krum as it names the median
    tr, get = make(DP_CLIP=1.0, DP_NOISE_MULTIPLIER=1.0, DP_DELTA=1e-5, DP_SEED=0)
    with pytest.raises(ValueError, match="FED.ROBUST_AGG"):
        tr._dp_cfg(get)


def test_abi_argument_checks_run_before_any_launch():
    """The new entry points' error returns, on the host: no device is touched."""
    from federated_multi_modal_amd import _lib, ops
    chunk = _lib.call("mf_krum_chunk_elems")
    assert chunk > 0 and chunk % 4 == 0 and ops.krum_chunk_elems() == chunk
    for args in ((0, 8), (65, 8), (3, -1)):
        assert _lib.call("mf_krum_ws_bytes", *args) == -1
    assert _lib.call("mf_krum_ws_bytes", 3, 0) > 0
    one = _lib.call("mf_krum_ws_bytes", 8, chunk)
    assert _lib.call("mf_krum_ws_bytes", 8, chunk + 1) == 2 * one     # a second chunk
    assert _lib.call("mf_krum_ws_bytes", 9, chunk) == 3 * one         # two client tiles: three pairs of tiles
    assert _lib.call("mf_krum_ws_bytes", 64, 3 * chunk) == 3 * 36 * one
    for args, text in (((None, 0, 8, 8, None, None, None), "nclients"),
                       ((None, 65, 8, 8, None, None, None), "nclients"),
                       ((None, 3, 7, 8, None, None, None), "stride"),
                       ((None, 3, 8, -1, None, None, None), "n < 0"),
                       ((None, 3, 8, 8, None, None, None), "null"),
                       ((None, 3, 8, 0, None, None, None), "null")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call("mf_krum_pairwise", *args)
    for args, text in (((None, 0, 3, 1, 0, None, None, None, None), "nparts"),
                       ((None, 1, 0, 1, 0, None, None, None, None), "nclients"),
                       ((None, 1, 65, 1, 0, None, None, None, None), "nclients"),
                       ((None, 1, 3, -1, 0, None, None, None, None), "f < 0"),
                       ((None, 1, 3, 1, -1, None, None, None, None), "m < 0"),
                       ((None, 1, 3, 1, 0, None, None, None, None), "null")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call("mf_krum_select", *args)
    for args, text in (((None, 65, 8, 8, None, -1, None, None), "nclients"),
                       ((None, 0, 8, 8, None, -1, None, None), "nclients"),
                       ((None, 3, 7, 8, None, -1, None, None), "stride"),
                       ((None, 3, 8, 8, None, 8, None, None), "count_pos"),
                       ((None, 3, 8, 8, None, -1, None, None), "null")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call("mf_fedavg_reduce_selected", *args)
    assert _lib.call("mf_fedavg_reduce_selected", None, 3, 8, 0, None, -1, None, None) == 0  # nothing to do
    # the wrappers' own checks, on CPU tensors
    g, out, sel = torch.zeros(3 * 8), torch.zeros(8), torch.zeros(3, dtype=torch.int32)
    ws, D = torch.zeros(64, dtype=torch.float64), torch.zeros(9, dtype=torch.float64)
    for kw, text in ((dict(nclients=65), "nclients"), (dict(count_pos=8), "count_pos"), (dict(out=g[:8]), "overlaps"),
                     (dict(selected=sel.float()), "selected"), (dict(selected=sel[:2]), "selected"),
                     (dict(gathered=g.double()), "gathered")):
        a = dict(gathered=g, nclients=3, selected=sel, count_pos=-1, out=out)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.fedavg_reduce_selected(a["gathered"], a["nclients"], a["selected"], a["count_pos"], a["out"])
    for kw, text in ((dict(nclients=0), "nclients"), (dict(n=9), "gathered"), (dict(ws=ws.float()), "ws"),
                     (dict(ws=ws[:1]), "ws"), (dict(dist=D[:8]), "dist"), (dict(dist=ws[:9]), "overlaps"),
                     (dict(gathered=g.half()), "gathered")):
        a = dict(gathered=g, nclients=3, n=8, ws=ws, dist=D)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.krum_pairwise(a["gathered"], a["nclients"], a["n"], a["ws"], a["dist"])
    sc, cnt = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    for kw, text in ((dict(nclients=65), "nclients"), (dict(f=-1), "f:"), (dict(m=-1), "m:"), (dict(m=True), "m:"),
                     (dict(parts=D[:8]), "parts"), (dict(parts=D.float()), "parts"), (dict(scores=sc[:2]), "scores"),
                     (dict(counts=cnt[:2]), "counts"), (dict(selected=cnt), "overlaps")):
        a = dict(parts=D, nclients=3, f=1, m=0, selected=sel, scores=sc, counts=cnt)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.krum_select(a["parts"], a["nclients"], a["f"], a["m"], a["selected"], a["scores"], a["counts"])
