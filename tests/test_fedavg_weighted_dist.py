"""CPU tier: sample-weighted FedAvg (McMahan et al., AISTATS 2017; FED.CLIENT_WEIGHTS) through the collective
protocol of federated_multi_modal_amd/federated.py on gloo ranks, with host restatements of the weighted pack /
unpack kernels (the GPU tier, tests/test_fedprox_weighted_gpu.py, checks the kernels against the same
restatements).  The layout mirrors tests/test_fedavg_dist.py, whose FakeEngine supplies the values: spread over
binades, so the fp32 summation order shows in the fp16 result.

Reference for the result, over the valid clients in client order, in torch on the CPU:
    acc = w0 * x0; acc += wc * xc ...;  ws = w0; ws += wc ...;  (acc / ws).half()
"""
import math

import pytest
import torch
import torch.distributed as dist

from test_fedavg_dist import FakeEngine, HostKernels, _init, _spawn


class WeightedHostKernels(HostKernels):
    """HostKernels plus the weighted pair: [fp32(w) * float(p) ... | w | 1], an invalid client all zeros; unpack
    divides by bucket[n] and reads the vote count at bucket[n + 1]."""

    @staticmethod
    def fedavg_pack_weighted(p16, p32, invalid, weight, bucket):
        n16, n32 = p16.numel(), p32.numel()
        assert bucket.numel() == n16 + n32 + 2
        if bool(invalid.item()):
            bucket.zero_()
            return
        w = torch.tensor(weight, dtype=torch.float32)
        bucket[:n16] = p16.float() * w
        bucket[n16:n16 + n32] = p32 * w
        bucket[n16 + n32] = w
        bucket[n16 + n32 + 1] = 1.0

    @staticmethod
    def fedavg_unpack_weighted(bucket, p16, p32, g16, g32):
        n16, n32 = p16.numel(), p32.numel()
        n = n16 + n32
        if float(bucket[n + 1]) == 0:
            p16.copy_(g16)
            p32.copy_(g32)
            return
        v = (bucket[:n] / bucket[n]).half()
        p16.copy_(v[:n16])
        p32.copy_(v[n16:].float())
        g16.copy_(p16)
        g32.copy_(p32)


def _valid(e):
    return bool(torch.isfinite(e.flat16.float()).all() and torch.isfinite(e.flat32).all())


def reference(clients, weights):
    """The torch CPU expression of the module docstring over the valid clients; None when there is none."""
    acc = ws = None
    for e, w in zip(clients, weights):
        if not _valid(e):
            continue
        x = torch.cat([e.flat16.float(), e.flat32])
        wt = torch.tensor(float(w), dtype=torch.float32)
        if acc is None:
            acc, ws = wt * x, wt.clone()
        else:
            acc += wt * x
            ws += wt
    if acc is None:
        return None
    v = (acc / ws).half()
    n16 = clients[0].n16
    return v[:n16], v[n16:].float()


def _prepared(client, bad, weight, mode):
    """A client's engine holding its local result, and its bucket built while it held the previous global weights."""
    from federated_multi_modal_amd.federated import FedAvgBucket
    e = FakeEngine(client, bad=client in bad)
    loc16, loc32 = e.flat16.clone(), e.flat32.clone()
    e.flat16.copy_(FakeEngine(0).flat16)
    e.flat32.copy_(FakeEngine(0).flat32)
    fed = FedAvgBucket(e, kernels=WeightedHostKernels, mode=mode, weight=weight)
    e.flat16.copy_(loc16)
    e.flat32.copy_(loc32)
    return e, fed


def _worker(rank, world, port, weights, bad, mode, out):
    _init(rank, world, port)
    e, fed = _prepared(rank, bad, None if weights is None else weights[rank], mode)
    n = e.n16 + e.n32
    tail = 1 if weights is None else 2
    assert fed.buf.numel() == n + tail and fed.pbuf.numel() == -(-(n + tail) // world) * world
    n_valid = fed.run()
    out[rank] = (n_valid, e.flat16.clone(), e.flat32.clone(), e.reloaded)
    dist.destroy_process_group()


@pytest.mark.parametrize("world,weights,bad", [(2, (3, 1), ()), (3, (3, 1, 2), ()),
                                               (3, (3, 1, 2), (1,)),   # rank 1 excluded: the denominator drops to 5
                                               (2, (3, 1), (0, 1))])   # nobody valid: the previous global weights
def test_weighted_ordered_exchange_is_bit_exact(world, weights, bad):
    res = _spawn(_worker, world, tuple(weights), tuple(bad), "ordered")
    clients = [FakeEngine(r, bad=r in bad) for r in range(world)]
    ref = reference(clients, weights)
    for r in range(world):
        n_valid, p16, p32, reloaded = res[r]
        assert n_valid == sum(_valid(c) for c in clients) and reloaded == 1
        if ref is None:
            assert n_valid == 0
            assert torch.equal(p16, FakeEngine(0).flat16) and torch.equal(p32, FakeEngine(0).flat32)
        else:
            assert torch.equal(p16, ref[0]) and torch.equal(p32, ref[1])


def test_equal_power_of_two_weights_are_the_unweighted_mean_bit_for_bit():
    """Scaling by 4 is exact in fp32 (no over- or underflow at these magnitudes), so weights (4, 4, 4) give the
    bits of the unweighted path; weights (3, 1, 2) do not (the test can fail)."""
    plain = _spawn(_worker, 3, None, (), "ordered")
    same = _spawn(_worker, 3, (4, 4, 4), (), "ordered")
    other = _spawn(_worker, 3, (3, 1, 2), (), "ordered")
    for r in range(3):
        assert plain[r][0] == same[r][0] == 3
        assert torch.equal(plain[r][1], same[r][1]) and torch.equal(plain[r][2], same[r][2])
    assert (plain[0][2] != other[0][2]).float().mean().item() > 0.5


def _group_worker(rank, world, port, per_rank, weights, mode, out):
    _init(rank, world, port)
    from federated_multi_modal_amd.federated import FedAvgExchange
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    pairs = [_prepared(c, (), weights[c], mode) for c in ids]
    feds = [f for _, f in pairs]
    x = FedAvgExchange(feds, mode=mode)
    for f in feds:
        f.pack()
    x.start()
    x.finish([])
    for f in feds:
        f.unpack()
    out[rank] = (x.n_valid(), [(e.flat16.clone(), e.flat32.clone()) for e, _ in pairs])
    dist.destroy_process_group()


def test_weighted_two_clients_per_rank():
    weights = (3, 1, 2, 5)
    res = _spawn(_group_worker, 2, 2, weights, "ordered")
    ref = reference([FakeEngine(c) for c in range(4)], weights)
    for r in range(2):
        n_valid, got = res[r]
        assert n_valid == 4
        for p16, p32 in got:
            assert torch.equal(p16, ref[0]) and torch.equal(p32, ref[1])


def test_weighted_allreduce_mode_within_one_fp16_ulp():
    """The collective's own summation order: within one fp16 ulp of the restatement, the bound of
    test_fedavg_dist.test_fedavg_exchange_matches_reference."""
    weights = (3, 1, 2)
    res = _spawn(_worker, 3, weights, (), "allreduce")
    ref16, ref32 = reference([FakeEngine(r) for r in range(3)], weights)
    ulp = torch.exp2(torch.floor(torch.log2(ref32.abs().clamp_min(2.0 ** -14))) - 10)
    ulp16 = torch.exp2(torch.floor(torch.log2(ref16.float().abs().clamp_min(2.0 ** -14))) - 10)
    for r in range(3):
        n_valid, p16, p32, _ = res[r]
        assert n_valid == 3
        assert ((p32 - ref32).abs() <= ulp).all()
        assert ((p16.float() - ref16.float()).abs() <= ulp16).all()


def test_late_failure_repack_carries_the_weight():
    """One process, three weighted buckets in one exchange: client 1 fails after it was packed, finish() packs
    again with its vote (and weight) withdrawn -> the (3, 2)-weighted mean of clients 0 and 2."""
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    weights = (3, 1, 2)
    pairs = [_prepared(c, (), weights[c], "ordered") for c in range(3)]
    feds = [f for _, f in pairs]
    x = FedAvgExchange(feds, mode="ordered")
    for f in feds:
        f.pack()
    x.start()
    x.finish([1])
    for f in feds:
        f.unpack()
    assert x.n_valid() == 2
    ref = reference([FakeEngine(0), FakeEngine(2)], (3, 2))
    for e, _ in pairs:
        assert torch.equal(e.flat16, ref[0]) and torch.equal(e.flat32, ref[1])
    # a weighted and an unweighted bucket of the same padded size never share an exchange
    e = FakeEngine(0, n32=(1 << 20) + 4)
    with pytest.raises(AssertionError):
        FedAvgExchange([feds[0], FedAvgBucket(e, kernels=WeightedHostKernels)], mode="ordered")
    with pytest.raises(ValueError):
        FedAvgBucket(FakeEngine(0), kernels=WeightedHostKernels, weight=0.0)


def test_resolve_client_weights():
    from federated_multi_modal_amd.federated import resolve_client_weights as R
    assert R("uniform", [], 3) is None
    assert R("uniform", [10, 20, 30], 3) is None
    assert R("samples", [10, 20, 30], 3) == [10.0, 20.0, 30.0]
    assert all(isinstance(w, float) for w in R("samples", [10, 20, 30], 3))
    assert R([3, 1, 2], [], 3) == [3.0, 1.0, 2.0]
    assert R((0.5, 1.5), [], 2) == [0.5, 1.5]
    assert R("3, 1,2", [], 3) == [3.0, 1.0, 2.0]
    assert R("samples", [2 ** 24 - 1, 1], 2) == [float(2 ** 24 - 1), 1.0]
    for spec, counts, n in [
        ([3, 1], [], 3), ("3,1", [], 3), ("samples", [10, 20], 3),          # wrong length
        ([3, 0, 2], [], 3), ([3, -1, 2], [], 3), ("samples", [10, 0, 5], 3),  # a weight <= 0
        ([3, math.inf, 2], [], 3), ([3, math.nan, 2], [], 3), ("1,nan", [], 2),  # non-finite
        ("samples", [2 ** 24, 5], 2),                                      # a count that is not exact in fp32
        ("sample", [1, 2], 2), (3.0, [], 1), (["a", "b"], [], 2),           # not a form at all
    ]:
        with pytest.raises(ValueError):
            R(spec, counts, n)


def test_config_keys_and_their_defaults():
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    cfg = get_cfg_default()
    extend_cfg(cfg)
    assert cfg.FED.CLIENT_WEIGHTS == "uniform" and cfg.FED.PROX_MU == 0.0
    # the forms a user writes: a name, a tuple (what "3,1,2" parses to on the command line), a YAML list
    cfg.merge_from_list(["FED.CLIENT_WEIGHTS", "samples", "FED.PROX_MU", 0.5])
    assert cfg.FED.CLIENT_WEIGHTS == "samples" and cfg.FED.PROX_MU == 0.5
    cfg.merge_from_list(["FED.CLIENT_WEIGHTS", "3,1,2", "FED.PROX_MU", 1])
    assert cfg.FED.CLIENT_WEIGHTS == (3, 1, 2) and cfg.FED.PROX_MU == 1.0
    cfg.merge_from_list(["FED.CLIENT_WEIGHTS", "uniform"])
    assert cfg.FED.CLIENT_WEIGHTS == "uniform"
    cfg.merge_from_other_cfg({"FED": {"CLIENT_WEIGHTS": [3, 1, 2]}})
    assert cfg.FED.CLIENT_WEIGHTS == (3, 1, 2)
    with pytest.raises(ValueError):
        cfg.merge_from_list(["FED.CLIENT_WEIGHTS", 3])
    with pytest.raises(ValueError):
        cfg.merge_from_list(["FED.AGGREGATION", "3,1,2"])  # the other keys keep yacs' type check


def test_host_safe_average_weights_weighted():
    """MaPLeFederated.safe_average_weights(weights=...) is the same expression on state dicts; without weights it
    is what it was."""
    from federated_multi_modal_amd.trainers import MaPLeFederated
    tr = MaPLeFederated.__new__(MaPLeFederated)
    clients = [FakeEngine(c, n32=4099) for c in range(3)]
    sds = [{"a": c.flat16, "b": c.flat32} for c in clients]
    got = tr.safe_average_weights(sds, weights=(3, 1, 2))
    ref16, ref32 = reference(clients, (3, 1, 2))
    assert torch.equal(got["a"], ref16) and torch.equal(got["b"].float(), ref32)
    plain = tr.safe_average_weights(sds)
    assert torch.equal(plain["b"], torch.stack([c.flat32 for c in clients]).mean(0).half())
    with pytest.raises(ValueError):
        tr.safe_average_weights(sds, weights=(3, 1))
