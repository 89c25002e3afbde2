"""CPU tier: robust aggregation (FED.ROBUST_AGG: the coordinate-wise median and trimmed mean of Yin, Chen,
Ramchandran and Bartlett, ICML 2018) through the collective protocol of federated_multi_modal_amd/federated.py on
gloo ranks, with host restatements of mf_fedavg_pack_robust / mf_fedavg_reduce_trimmed in the kernels' place (the GPU
tier, tests/test_fedavg_robust_gpu.py, checks the kernels against the same restatements bit for bit).

host_trimmed is the restatement of the contract in include/mapfed.h, in torch on the CPU: a sort of the int32 keys of
the IEEE total order, then predicated sequential fp32 adds that start from the first kept value, then one division.
A sum taken in sorted order depends on neither the client order, the world size nor the clients per rank, so every
layout of a client set must give the bits of host_trimmed over all its clients' buckets in one process."""
import pytest
import torch
import torch.distributed as dist

from test_fedavg_dist import FakeEngine, _init, _spawn
from test_fedavg_weighted_dist import WeightedHostKernels

N16, N32 = 37, 4096 + 3
N = N16 + N32
QNAN_BITS = 0x7FC00000
ABSENT_KEY = 0x7FFFFFFF
MEDIAN_TRIM = 2 ** 31 - 1


def _order_key(bits):
    """bits (int32) -> the key whose signed order is the IEEE total order; its own inverse."""
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)


def host_trimmed(g, trim_k, count_pos=-1):
    """g: [clients, n] fp32 on the CPU.  Per coordinate: NaN = absent, m present values sorted in the total order,
    k = min(trim_k, (m - 1) // 2) cut at either end, the kept ones summed in ascending order from the first kept
    value, divided by m - 2k; m = 0 gives +0; out[count_pos] = m."""
    g = g.detach().contiguous()
    clients, n = g.shape
    absent = torch.isnan(g)
    key = torch.where(absent, torch.full((), ABSENT_KEY, dtype=torch.int32), _order_key(g.view(torch.int32)))
    m = (~absent).sum(0)
    s = _order_key(torch.sort(key, dim=0).values).view(torch.float32)  # absent (the largest key) last
    k = torch.minimum(torch.full_like(m, min(int(trim_k), MEDIAN_TRIM)),
                      torch.div(m - 1, 2, rounding_mode="floor")).clamp_min(0)
    end = m - k
    acc = torch.zeros(n, dtype=torch.float32)
    for p in range(clients):
        acc = torch.where(k == p, s[p], torch.where((k < p) & (p < end), acc + s[p], acc))
    out = torch.where(m == 0, torch.zeros(n, dtype=torch.float32), acc / (m - 2 * k).float())
    if count_pos >= 0:
        out[count_pos] = float(m[count_pos])
    return out


class RobustHostKernels(WeightedHostKernels):
    """The host kernels plus the robust pair, with ops.fedavg_pack_robust's / ops.fedavg_reduce_trimmed's signatures:
    [float(p) ... | 1 | 1], an invalid client all quiet NaNs (0x7fc00000)."""

    @staticmethod
    def fedavg_pack_robust(p16, p32, invalid, bucket):
        n16, n32 = p16.numel(), p32.numel()
        assert bucket.numel() == n16 + n32 + 2
        if bool(invalid.item()):
            bucket.view(torch.int32).fill_(QNAN_BITS)
            return
        bucket[:n16] = p16.float()
        bucket[n16:n16 + n32] = p32
        bucket[n16 + n32:] = 1.0

    @staticmethod
    def fedavg_reduce_trimmed(gathered, nclients, trim_k, count_pos, out):
        g = gathered.view(nclients, -1)[:, :out.numel()]
        out.copy_(host_trimmed(g, trim_k, count_pos))


AGGS = (("median", 1), ("trimmed_mean", 1), ("trimmed_mean", 2))


def scenarios(n):
    """name -> (invalid clients, finite outliers, clients that fail after they were packed)."""
    return {"clean": ((), (), ()), "bad": ((1,), (), ()), "outlier": ((), (0,), ()), "late": ((), (), (n - 1,)),
            "nobody": (tuple(range(n)), (), ())}


def client_engine(c, bad=(), outlier=()):
    e = FakeEngine(c, n16=N16, n32=N32, bad=c in bad)
    if c in outlier:  # finite but wrong: what the validity scan lets through
        e.flat16.mul_(-40.0)
        e.flat32.mul_(-1000.0)
    return e


def global_engine():
    return FakeEngine(0, n16=N16, n32=N32)


def expected(n, robust, trim_k, bad, outlier, late):
    """The single-process restatement over all n clients: (n_valid, fp32 statistic or None, flat16, flat32)."""
    from federated_multi_modal_amd.federated import robust_trim
    rows = []
    for c in range(n):
        e = client_engine(c, bad, outlier)
        row = torch.cat([e.flat16.float(), e.flat32, torch.ones(2)])
        if c in bad or c in late:
            row = torch.full_like(row, float("nan"))
        rows.append(row)
    red = host_trimmed(torch.stack(rows), robust_trim(robust, trim_k), N + 1)
    m = int(red[N + 1])
    assert float(red[N]) == (1.0 if m else 0.0)  # the statistic of all-ones is exactly 1
    if m == 0:
        g = global_engine()
        return 0, None, g.flat16, g.flat32
    v = (red[:N] / red[N]).half()
    return m, red[:N], v[:N16], v[N16:].float()


def run_round(ids, robust, trim_k, bad, outlier, late, kernels=RobustHostKernels):
    """The clients `ids` of this process through one FedAvgExchange: pack, exchange, (late failures,) unpack."""
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    engines, feds = [], []
    for c in ids:
        e = client_engine(c, bad, outlier)
        loc16, loc32 = e.flat16.clone(), e.flat32.clone()
        e.flat16.copy_(global_engine().flat16)  # the bucket's global copy: the previous global weights
        e.flat32.copy_(global_engine().flat32)
        feds.append(FedAvgBucket(e, kernels=kernels, robust=robust, trim_k=trim_k))
        e.flat16.copy_(loc16)
        e.flat32.copy_(loc32)
        engines.append(e)
    assert all(f.buf.numel() == N + 2 for f in feds)
    x = FedAvgExchange(feds, robust=robust, trim_k=trim_k)
    for f in feds:
        f.pack()
    x.start()
    x.finish([j for j, c in enumerate(ids) if c in late])
    stat = feds[0].buf[:N].clone()
    for f in feds:
        f.unpack()
    return x.n_valid(), stat, [(e.flat16.clone(), e.flat32.clone()) for e in engines]


def _worker(rank, world, port, per_rank, out):
    _init(rank, world, port)
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    res = {}
    for robust, trim_k in AGGS:
        for name, (bad, outlier, late) in scenarios(world * per_rank).items():
            res[(robust, trim_k, name)] = run_round(ids, robust, trim_k, bad, outlier, late)
    out[rank] = res
    dist.destroy_process_group()


@pytest.mark.parametrize("world,per_rank", [(2, 1), (3, 1), (8, 1), (2, 2), (3, 2)])
def test_robust_exchange_is_bit_exact_at_every_layout(world, per_rank):
    """Median and trimmed mean (trim 1 and 2), with no bad client, an invalid one, a finite outlier, a late failure
    and nobody valid: every client of every rank ends with the restatement's weights, the fp32 statistic itself
    equals it bit for bit, and the same client set in one process (the non-distributed path) gives the same bits."""
    n = world * per_rank
    res = _spawn(_worker, world, per_rank)
    for robust, trim_k in AGGS:
        for name, (bad, outlier, late) in scenarios(n).items():
            n_valid, stat, ref16, ref32 = expected(n, robust, trim_k, bad, outlier, late)
            assert n_valid == n - len(bad) - len(late)
            one = run_round(list(range(n)), robust, trim_k, bad, outlier, late)  # one process, n clients
            for got_valid, got_stat, weights in [res[r][(robust, trim_k, name)] for r in range(world)] + [one]:
                assert got_valid == n_valid, (robust, trim_k, name)
                if stat is not None:
                    assert torch.equal(got_stat.view(torch.int32), stat.view(torch.int32)), (robust, trim_k, name)
                for p16, p32 in weights:
                    assert torch.equal(p16, ref16) and torch.equal(p32, ref32), (robust, trim_k, name)
            if name == "nobody":  # the round is skipped: the previous global weights
                assert n_valid == 0
                assert torch.equal(ref16, global_engine().flat16) and torch.equal(ref32, global_engine().flat32)


def test_restatement_on_known_columns():
    """host_trimmed against values worked out by hand, and against torch.median for odd m."""
    nan, inf = float("nan"), float("inf")
    g = torch.tensor([[1.0, 5.0, -0.0, nan, 3.0, 1.0],
                      [2.0, 1.0, 0.0, nan, nan, inf],
                      [9.0, 3.0, -0.0, nan, 1.0, 2.0],
                      [4.0, 7.0, 0.0, nan, -nan, 3.0]])
    med = host_trimmed(g, MEDIAN_TRIM)
    assert med.tolist()[:2] == [3.0, 4.0]                      # even m: the mean of the two middle values
    assert med[2].item() == 0.0 and not torch.signbit(med[2])  # (-0 + +0) / 2
    assert med[3].item() == 0.0 and not torch.signbit(med[3])  # nobody present: +0
    assert med[4].item() == 2.0 and med[5].item() == 2.5       # m = 2 of 4; +Inf is present and trimmed away
    assert host_trimmed(g, 0)[5].item() == inf
    t1 = host_trimmed(g, 1, count_pos=4)
    assert t1.tolist()[:2] == [3.0, 4.0] and t1[4].item() == 2.0  # m at the count element
    assert torch.signbit(host_trimmed(torch.tensor([[-0.0], [nan]]), 0))[0]  # a lone -0 stays -0
    x = torch.randn(7, 501)
    assert torch.equal(host_trimmed(x, MEDIAN_TRIM), x.median(0).values)
    assert torch.equal(host_trimmed(x, 3), x.median(0).values)
    perm = torch.randperm(7)
    assert torch.equal(host_trimmed(x, 2), host_trimmed(x[perm], 2))
    # trim 0 is a mean in sorted order: close to, and not everywhere equal to, the client-order mean
    y = torch.randn(8, 4096) * torch.exp2(torch.randint(-6, 6, (8, 4096)).float())
    a, b = host_trimmed(y, 0), y.sum(0) / 8
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_robust_resists_outliers_where_the_mean_does_not():
    """8 clients, 2 of them with values of magnitude 6e4 and random sign: the median and the 2-trimmed mean of every
    coordinate lie within the honest clients' [min, max] (exact inequalities), the untrimmed mean does not."""
    g = torch.Generator().manual_seed(5)
    honest = torch.randn(6, 2000, generator=g)
    wrong = 6e4 * (torch.randint(0, 2, (2, 2000), generator=g).float() * 2 - 1)
    x = torch.cat([honest[:3], wrong[:1], honest[3:], wrong[1:]])
    lo, hi = honest.min(0).values, honest.max(0).values
    for trim in (MEDIAN_TRIM, 2):
        r = host_trimmed(x, trim)
        assert ((lo <= r) & (r <= hi)).all()
    r0 = host_trimmed(x, 0)
    assert not ((lo <= r0) & (r0 <= hi)).all()


def test_construction_errors():
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    e = global_engine()
    K = RobustHostKernels
    with pytest.raises(ValueError, match="allreduce"):
        FedAvgBucket(e, kernels=K, mode="allreduce", robust="median")
    with pytest.raises(ValueError, match="weight"):
        FedAvgBucket(e, kernels=K, weight=2.0, robust="median")
    with pytest.raises(ValueError, match="krum"):
        FedAvgBucket(e, kernels=K, robust="krum")
    for bad_k in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="trim_k"):
            FedAvgBucket(e, kernels=K, robust="trimmed_mean", trim_k=bad_k)
    FedAvgBucket(e, kernels=K, robust="median", trim_k=0)  # the median takes no trim
    fed = FedAvgBucket(e, kernels=K, robust="trimmed_mean", trim_k=1)
    with pytest.raises(ValueError, match="allreduce"):
        FedAvgExchange([fed], mode="allreduce", robust="trimmed_mean", trim_k=1)
    with pytest.raises(ValueError, match="krum"):
        FedAvgExchange([fed], robust="krum")
    with pytest.raises(ValueError, match="trim_k"):
        FedAvgExchange([fed], robust="trimmed_mean", trim_k=0)
    with pytest.raises(AssertionError):  # a bucket and an exchange that disagree
        FedAvgExchange([fed], robust="median")
    with pytest.raises(AssertionError):
        FedAvgExchange([fed])
    # without robust the host kernels of the other test files (no robust attributes) still serve
    from test_fedavg_dist import HostKernels
    plain = FedAvgBucket(global_engine(), kernels=HostKernels)
    assert plain.run() == 1 and plain.buf.numel() == N + 1


def test_config_keys_and_trainer_validation(capsys):
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    from federated_multi_modal_amd.trainers import MaPLeFederated
    cfg = get_cfg_default()
    extend_cfg(cfg)
    assert cfg.FED.ROBUST_AGG == "none" and cfg.FED.TRIM_K == 1
    cfg.merge_from_list(["FED.ROBUST_AGG", "trimmed_mean", "FED.TRIM_K", 2])
    assert cfg.FED.ROBUST_AGG == "trimmed_mean" and cfg.FED.TRIM_K == 2

    def check(num_clients=8, rank=0, **keys):
        tr = MaPLeFederated.__new__(MaPLeFederated)
        tr.num_clients, tr.rank = num_clients, rank
        fed = {"ROBUST_AGG": "none", "TRIM_K": 1, "AGGREGATION": "ordered", "CLIENT_WEIGHTS": "uniform"}
        fed.update(keys)
        return tr._robust_cfg(fed.get)

    assert check() == (None, 1)
    assert check(ROBUST_AGG="median") == ("median", 1)
    assert "median" in capsys.readouterr().out
    assert check(ROBUST_AGG="Trimmed_Mean", TRIM_K=3) == ("trimmed_mean", 3)
    assert "[INFO] Robust aggregation" in capsys.readouterr().out
    check(ROBUST_AGG="median", rank=1)
    assert capsys.readouterr().out == ""  # rank 0 alone reports
    assert check(ROBUST_AGG="median", TRIM_K=7, num_clients=3) == ("median", 7)  # the median ignores the trim
    for key, keys in (("FED.ROBUST_AGG", dict(ROBUST_AGG="krum")),
                      ("FED.TRIM_K", dict(TRIM_K=0)),
                      ("FED.TRIM_K", dict(ROBUST_AGG="trimmed_mean", TRIM_K=-1)),
                      ("FED.TRIM_K", dict(ROBUST_AGG="trimmed_mean", TRIM_K=4)),           # 2 * 4 >= 8 clients
                      ("FED.TRIM_K", dict(ROBUST_AGG="trimmed_mean", TRIM_K=1, num_clients=2)),
                      ("FED.NUM_CLIENTS", dict(ROBUST_AGG="median", num_clients=65)),
                      ("FED.AGGREGATION", dict(ROBUST_AGG="median", AGGREGATION="allreduce")),
                      ("FED.CLIENT_WEIGHTS", dict(ROBUST_AGG="median", CLIENT_WEIGHTS="samples")),
                      ("FED.CLIENT_WEIGHTS", dict(ROBUST_AGG="trimmed_mean", CLIENT_WEIGHTS=(3, 1, 2)))):
        with pytest.raises(ValueError, match=key):
            check(**keys)
    assert check(ROBUST_AGG="trimmed_mean", TRIM_K=3) == ("trimmed_mean", 3)  # 2 * 3 < 8


def test_abi_argument_checks_run_before_any_launch():
    """mf_fedavg_reduce_trimmed's error returns, on the host: no device is touched."""
    from federated_multi_modal_amd import _lib, ops
    for args, text in (((None, 65, 8, 8, 0, -1, None, None), "nclients"),
                       ((None, 0, 8, 8, 0, -1, None, None), "nclients"),
                       ((None, 3, 8, 8, -1, -1, None, None), "trim_k"),
                       ((None, 3, 7, 8, 0, -1, None, None), "stride"),
                       ((None, 3, 8, 8, 0, 8, None, None), "count_pos")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call("mf_fedavg_reduce_trimmed", *args)
    assert _lib.call("mf_fedavg_reduce_trimmed", None, 3, 8, 0, 0, -1, None, None) == 0  # nothing to do
    g, out = torch.zeros(3 * 8), torch.zeros(8)
    for kw, text in ((dict(nclients=65), "nclients"), (dict(trim_k=-1), "trim_k"), (dict(count_pos=8), "count_pos"),
                     (dict(out=g[:8]), "overlaps")):
        a = dict(gathered=g, nclients=3, trim_k=0, count_pos=-1, out=out)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.fedavg_reduce_trimmed(a["gathered"], a["nclients"], a["trim_k"], a["count_pos"], a["out"])
