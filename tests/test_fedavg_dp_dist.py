"""CPU tier: DP-FedAvg (FED.DP_CLIP / FED.DP_NOISE_MULTIPLIER: per-client update clipping and Gaussian noise, McMahan,
Ramage, Talwar and Zhang, ICLR 2018) through the collective protocol of federated_multi_modal_amd/federated.py on
gloo ranks, with host restatements of mf_dp_update_scale / mf_fedavg_pack_clipped / mf_dp_add_noise in the kernels'
place (the GPU tier, tests/test_fedavg_dp_gpu.py, checks the kernels against the same restatements).

The noise at global coordinate i is a function of (seed, round, i) alone -- Philox4x32-10 on the counter
(i >> 2, round) under the key seed, Box-Muller on its words -- so rank r noises its own shard of the sum and every
layout of a client set must end with the bits of one process over all its clients."""
import math

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_fedavg_dist import FakeEngine, HostKernels, _init, _spawn
from test_fedavg_robust_dist import QNAN_BITS, RobustHostKernels

N16, N32 = 37, 4096 + 3
N = N16 + N32
CLIP = 0.5
Z = 1.1
STD = float(np.float32(Z) * np.float32(CLIP))
SEED = 0x1234_5678_9ABC_DEF0  # both key words in use

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC 2011) on uint64 numpy arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0, p1 = c0 * np.uint64(M0), c2 * np.uint64(M1)  # 32 x 32 -> 64 bits, exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _uniform_words(i, seed, rnd):
    """Global coordinates i (uint64 array) -> the two Philox words (a, b) each one's normal is made of."""
    i = np.asarray(i, dtype=np.uint64)
    q, lane = i >> np.uint64(2), (i & np.uint64(3)).astype(np.int64)
    x = philox4x32_10(q & MASK, q >> np.uint64(32), np.full_like(q, rnd), np.zeros_like(q), seed & MASK, seed >> 32)
    a = np.where(lane < 2, x[0], x[2])
    b = np.where(lane < 2, x[1], x[3])
    return a, b, lane


def _unit(x):
    """float(((x >> 9) << 1) | 1) * 2^-24: an odd multiple of 2^-24 in (0, 1), exact in fp32."""
    return ((((x >> np.uint64(9)) << np.uint64(1)) | np.uint64(1)).astype(np.float32)) * np.float32(2.0 ** -24)


def host_normals(i, seed, rnd):
    """z(i) as the contract of include/mapfed.h states it, in numpy fp32."""
    a, b, lane = _uniform_words(i, seed, rnd)
    r = np.sqrt(np.float32(-2.0) * np.log(_unit(a)))
    theta = np.float32(6.2831855) * _unit(b)
    return np.where(lane % 2 == 0, r * np.cos(theta), r * np.sin(theta)).astype(np.float32)


def host_normals64(i, seed, rnd):
    """The fp64 Box-Muller of the same exact uniforms (the GPU tier's accuracy reference)."""
    a, b, lane = _uniform_words(i, seed, rnd)
    r = np.sqrt(-2.0 * np.log(_unit(a).astype(np.float64)))
    theta = 2.0 * np.pi * _unit(b).astype(np.float64)
    return np.where(lane % 2 == 0, r * np.cos(theta), r * np.sin(theta))


def host_update_scale(p16, g16, p32, g32, clip):
    """(norm, scale, clipped) in fp32: the fp64 norm of the fp32 differences, rounded; scale = clip / norm above."""
    d = torch.cat([p16.float() - g16.float(), p32 - g32])
    norm = torch.sqrt((d.double() ** 2).sum()).float()
    c = torch.tensor(clip, dtype=torch.float32)
    clipped = bool(norm > c)
    return norm, (c / norm if clipped else torch.ones((), dtype=torch.float32)), clipped


def host_clipped(p16, p32, g16, g32, s):
    """[y]: float(p) when s >= 1, else g + s * (float(p) - float(g)), three fp32 operations."""
    x, g = torch.cat([p16.float(), p32]), torch.cat([g16.float(), g32])
    if float(s) >= 1.0:
        return x
    d = x - g
    sd = d * torch.as_tensor(s, dtype=torch.float32)
    return g + sd


class DPHostKernels(RobustHostKernels):
    """The host kernels plus the DP-FedAvg three, with the signatures of ops.dp_update_scale,
    ops.fedavg_pack_clipped and ops.dp_add_noise."""

    @staticmethod
    def dp_update_ws_floats(n16, n32):
        return 1

    @staticmethod
    def dp_update_scale(p16, g16, p32, g32, clip, ws, out):
        norm, scale, clipped = host_update_scale(p16, g16, p32, g32, clip)
        out[0], out[1], out[2] = norm, scale, float(clipped)

    @staticmethod
    def fedavg_pack_clipped(p16, p32, g16, g32, invalid, scale, weight, layout, bucket):
        n = p16.numel() + p32.numel()
        assert bucket.numel() == n + (1 if layout == "plain" else 2)
        if bool(invalid.item()):
            if layout == "robust":
                bucket.view(torch.int32).fill_(QNAN_BITS)
            else:
                bucket.zero_()
            return
        y = host_clipped(p16, p32, g16, g32, scale[0])
        if layout == "weighted":
            w = torch.tensor(weight, dtype=torch.float32)
            bucket[:n] = y * w
            bucket[n] = w
        else:
            bucket[:n] = y
            bucket[n] = 1.0
        bucket[n + 1 if layout != "plain" else n] = 1.0

    @staticmethod
    def dp_add_noise(buf, offset, seed, rnd, std):
        if std == 0.0 or buf.numel() == 0:
            return
        z = host_normals(np.uint64(offset) + np.arange(buf.numel(), dtype=np.uint64), seed, rnd)
        buf.add_(torch.from_numpy(np.float32(std) * z))


# ----------------------------------------------------------------------------- the generator itself

def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 at 10 rounds."""
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((MASK,) * 4, (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = philox4x32_10(*[np.array([c]) for c in ctr], *key)
        assert tuple(int(g[0]) for g in got) == want


def test_host_normals_are_counter_based():
    i = np.arange(5000, dtype=np.uint64)
    z = host_normals(i, SEED, 3)
    assert np.array_equal(z[1237:2001], host_normals(i[1237:2001], SEED, 3))  # any split gives the same values
    assert not np.array_equal(z, host_normals(i, SEED, 4)) and not np.array_equal(z, host_normals(i, SEED + 1, 3))
    u = _unit(np.array([0, MASK], dtype=np.uint64))
    assert u[0] == 2.0 ** -24 and u[1] == 1.0 - 2.0 ** -24
    assert np.abs(z - host_normals64(i, SEED, 3)).max() < 2e-5
    hi = np.uint64(2 ** 34) + i  # the counter's high word in use
    assert not np.array_equal(host_normals(hi, SEED, 3), z)


# ----------------------------------------------------------------------------- every layout, one set of bits

def scenarios(n):
    """name -> (invalid clients, clients 100 x further out, clients that fail after they were packed)."""
    return {"clean": ((), (), ()), "bad": ((1,), (), ()), "late": ((), (), (n - 1,)),
            "nobody": (tuple(range(n)), (), ()), "big": ((), (0,), ())}


def global_engine():
    return FakeEngine(0, n16=N16, n32=N32)


def client_engine(c, bad=(), big=()):
    """The global weights plus a small update (L2 norm about 0.09, below 0.12: inside CLIP), 100 x as large for `big`."""
    e, g = global_engine(), torch.Generator().manual_seed(500 + c)
    f = 100.0 if c in big else 1.0
    e.flat16 = (e.flat16.float() + f * 1e-2 * torch.randn(N16, generator=g)).half()
    e.flat32 = e.flat32 + f * 1e-3 * torch.randn(N32, generator=g)
    if c in bad:
        e.flat32[3] = float("nan")
    return e


def expected(n, bad, big, late, rnd=0, std=STD):
    """One process, no exchange: (n_valid, fp32 noised sum, flat16, flat32, scales)."""
    glob = global_engine()
    acc, scales, m = None, [], 0
    for c in range(n):
        e = client_engine(c, bad, big)
        _, s, _ = host_update_scale(e.flat16, glob.flat16, e.flat32, glob.flat32, CLIP)
        scales.append(float(s))
        if c in bad or c in late:
            row = torch.zeros(N)
        else:
            row, m = host_clipped(e.flat16, e.flat32, glob.flat16, glob.flat32, s), m + 1
        acc = row.clone() if acc is None else acc + row
    DPHostKernels.dp_add_noise(acc, 0, SEED, rnd, std)
    if m == 0:
        return 0, acc, glob.flat16, glob.flat32, scales
    v = (acc / torch.tensor(float(m))).half()
    return m, acc, v[:N16], v[N16:].float(), scales


def build(ids, bad=(), big=(), kernels=DPHostKernels, dp_clip=CLIP, dp_std=STD, engine=client_engine, **kw):
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    engines, feds = [], []
    for c in ids:
        e = engine(c, bad, big)
        loc16, loc32 = e.flat16.clone(), e.flat32.clone()
        e.flat16.copy_(global_engine().flat16)  # the bucket's global copy: the weights the round started from
        e.flat32.copy_(global_engine().flat32)
        w = kw.get("weights")
        feds.append(FedAvgBucket(e, kernels=kernels, dp_clip=dp_clip, robust=kw.get("robust"),
                                 weight=None if w is None else w[c]))
        e.flat16.copy_(loc16)
        e.flat32.copy_(loc32)
        engines.append(e)
    xkw = dict(dp_std=dp_std, dp_seed=SEED) if dp_clip is not None else {}
    return engines, feds, FedAvgExchange(feds, robust=kw.get("robust"), **xkw)


def run_round(ids, bad, big, late):
    engines, feds, x = build(ids, bad, big)
    for f in feds:
        f.pack()
    x.start()
    x.finish([j for j, c in enumerate(ids) if c in late])
    assert x.round == 1 and x.state_dict() == {"round": 1, "seed": SEED}
    stat = feds[0].buf[:N].clone()
    stats = [f.clip_stats() for f in feds]
    for f in feds:
        f.unpack()
    return x.n_valid(), stat, [(e.flat16.clone(), e.flat32.clone()) for e in engines], stats


def _worker(rank, world, port, per_rank, out):
    _init(rank, world, port)
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    out[rank] = {name: run_round(ids, *sc) for name, sc in scenarios(world * per_rank).items()}
    dist.destroy_process_group()


@pytest.mark.parametrize("world,per_rank", [(2, 1), (3, 1), (8, 1), (2, 2), (3, 2)])
def test_dp_exchange_is_bit_exact_at_every_layout(world, per_rank):
    """Clean, an invalid client, a late failure (the re-exchange noised with the same round's stream), nobody valid
    and one client 100 x further out than the others: every layout ends with the restatement's fp32 noised sum and
    fp16 weights bit for bit, and so does the same client set in one process.  At world 3 the shard size is odd, so
    the shards' offsets are no multiples of 4."""
    n = world * per_rank
    if world == 3:
        assert (-(-(N + 1) // 3)) % 2 == 1
    res = _spawn(_worker, world, per_rank)
    for name, (bad, big, late) in scenarios(n).items():
        n_valid, stat, ref16, ref32, scales = expected(n, bad, big, late)
        assert n_valid == n - len(bad) - len(late), name
        one = run_round(list(range(n)), bad, big, late)
        for r, (got_valid, got_stat, weights, stats) in [(r, res[r][name]) for r in range(world)] + [(None, one)]:
            assert got_valid == n_valid, name
            assert torch.equal(got_stat.view(torch.int32), stat.view(torch.int32)), (name, r)
            for p16, p32 in weights:
                assert torch.equal(p16, ref16) and torch.equal(p32, ref32), (name, r)
            ids = range(n) if r is None else range(r * per_rank, (r + 1) * per_rank)
            for c, (norm, scale) in zip(ids, stats):
                if c in bad:
                    continue  # a NaN norm: scale 1, and the validity flag excludes the client
                assert scale == scales[c] and (scale < 1.0) == (c in big), (name, c, norm, scale)
                assert (norm > CLIP) == (c in big)
        if name == "nobody":
            assert torch.equal(ref16, global_engine().flat16) and torch.equal(ref32, global_engine().flat32)
        if name == "big":  # the clipped client moved the sum by at most CLIP (plus the rounding of g + s * delta)
            clean = expected(n, (), (), (), std=0.0)[1]
            noiseless = expected(n, bad, big, late, std=0.0)[1]
            assert (noiseless - clean).double().norm() <= CLIP * (1 + 1e-5) + 0.12 + math.sqrt(N) * 2.0 ** -24 * 40


def test_round_counter_and_noise_streams():
    """finish() advances the round once (also over a late-failure re-exchange); the same inputs a round later get
    other noise; a restored state continues the stream."""
    engines, feds, x = build([0, 1, 2])
    sums = []
    for rnd in range(3):
        for e, c in zip(engines, range(3)):  # the same inputs and the same global copy every round
            e.flat16.copy_(client_engine(c).flat16)
            e.flat32.copy_(client_engine(c).flat32)
        for f in feds:
            f.pack()
        x.start()
        x.finish([2] if rnd == 1 else [])
        assert x.round == rnd + 1
        sums.append(feds[0].buf[:N].clone())
        want = expected(3, (), (), (2,) if rnd == 1 else (), rnd=rnd)[1]
        assert torch.equal(sums[-1].view(torch.int32), want.view(torch.int32)), rnd
    assert not torch.equal(sums[0], sums[2])  # rounds 0 and 2: the same clipped sum, other noise
    assert torch.equal(expected(3, (), (), (), std=0.0)[1], expected(3, (), (), (), rnd=2, std=0.0)[1])
    sd = x.state_dict()
    assert sd == {"round": 3, "seed": SEED}
    _, feds2, y = build([0, 1, 2])
    y.load_state_dict({"round": 2, "seed": SEED})
    for f in feds2:
        f.pack()
    y.start()
    y.finish()
    assert y.round == 3 and torch.equal(feds2[0].buf[:N].view(torch.int32), sums[2].view(torch.int32))
    for bad_sd in ({"round": -1, "seed": 0}, {"round": 0}, {"round": 1.5, "seed": 0}, {"round": 0, "seed": 2 ** 64}):
        with pytest.raises(ValueError, match="state"):
            y.load_state_dict(bad_sd)


def _fake(c, bad=(), big=()):
    return FakeEngine(c, n16=N16, n32=N32, bad=c in bad)


@pytest.mark.parametrize("kw", [{}, {"weights": (3.0, 1.0, 2.0)}, {"robust": "median"}])
def test_a_bound_nobody_reaches_is_the_plain_exchange(kw):
    """dp_clip = 1e30, dp_std = 0: the select packs the weights themselves, so the summed bucket and the weights carry
    the bits of the exchange without DP -- plain, with client weights and under the median."""
    outs = []
    for dp_clip in (1e30, None):
        engines, feds, x = build([0, 1, 2], bad=(1,), dp_clip=dp_clip, dp_std=0.0, engine=_fake, **kw)
        for f in feds:
            f.pack()
        if dp_clip is not None:
            assert feds[2].clip_stats()[1] == 1.0 and feds[2].clip_stats()[0] > 10.0
        x.start()
        x.finish()
        total = feds[0].buf.clone()
        for f in feds:
            f.unpack()
        outs.append((x.n_valid(), total, [(e.flat16.clone(), e.flat32.clone()) for e in engines]))
    (va, ta, wa), (vb, tb, wb) = outs
    assert va == vb == 2 and torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    for (a16, a32), (b16, b32) in zip(wa, wb):
        assert torch.equal(a16, b16) and torch.equal(a32, b32)


def test_clipping_combines_with_weights_and_the_median():
    """dp_clip alone, a bound every client exceeds: the weighted mean and the median of the clipped weights."""
    from test_fedavg_robust_dist import MEDIAN_TRIM, host_trimmed
    glob, ws = global_engine(), {1: 3.0, 2: 1.0, 3: 2.0}  # client 0 of FakeEngine holds the global weights themselves
    ys = []
    for c in (1, 2, 3):
        e = _fake(c)
        _, s, clipped = host_update_scale(e.flat16, glob.flat16, e.flat32, glob.flat32, CLIP)
        assert clipped
        ys.append(host_clipped(e.flat16, e.flat32, glob.flat16, glob.flat32, s))
        assert (ys[-1] - torch.cat([glob.flat16.float(), glob.flat32])).double().norm() <= CLIP * (1 + 1e-5) + 1e-4
    for kw in ({"weights": ws}, {"robust": "median"}):
        engines, feds, x = build([1, 2, 3], dp_std=0.0, engine=_fake, **kw)
        for f in feds:
            f.pack()
        x.start()
        x.finish()
        if "weights" in kw:
            acc = ys[0] * ws[1]
            for w, y in zip((ws[2], ws[3]), ys[1:]):
                acc = acc + y * w
            want = acc
        else:
            want = host_trimmed(torch.stack(ys), MEDIAN_TRIM)
        assert torch.equal(feds[0].buf[:N].view(torch.int32), want.view(torch.int32)), kw


# ----------------------------------------------------------------------------- accountant, errors, config

def test_accountant():
    from federated_multi_modal_amd.federated import dp_epsilon
    for z, rounds, delta in ((1.1, 30, 1e-5), (0.5, 1, 1e-5), (4.0, 1000, 1e-7), (0.8, 7, 1e-3)):
        a_star = 1.0 + z * math.sqrt(2.0 * math.log(1.0 / delta) / rounds)
        alpha = 1.0 + (a_star - 1.0) * np.exp(np.linspace(-3.0, 3.0, 2_000_001))  # fine, and dense at the minimum
        grid = (rounds * alpha / (2.0 * z * z) + math.log(1.0 / delta) / (alpha - 1.0)).min()
        assert abs(dp_epsilon(z, rounds, delta) - grid) <= 1e-6 * grid, (z, rounds, delta)
    assert dp_epsilon(0.0, 5, 1e-5) == math.inf and dp_epsilon(1.0, 0, 1e-5) == 0.0
    eps = [dp_epsilon(z, 30, 1e-5) for z in (0.3, 0.6, 1.0, 2.0, 8.0)]
    assert all(a > b for a, b in zip(eps, eps[1:]))
    assert dp_epsilon(1.0, 31, 1e-5) > dp_epsilon(1.0, 30, 1e-5)
    for args in ((-1.0, 1, 1e-5), (1.0, -1, 1e-5), (1.0, 1.5, 1e-5), (1.0, 1, 0.0), (1.0, 1, 1.0),
                 (float("nan"), 1, 1e-5)):
        with pytest.raises(ValueError, match="dp_epsilon"):
            dp_epsilon(*args)


def test_construction_errors():
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    K = DPHostKernels
    for bad_clip in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="dp_clip"):
            FedAvgBucket(global_engine(), kernels=K, dp_clip=bad_clip)
    clipped = FedAvgBucket(global_engine(), kernels=K, dp_clip=1.0)
    plain = FedAvgBucket(global_engine(), kernels=K)
    with pytest.raises(ValueError, match="dp_clip on every bucket"):
        FedAvgExchange([clipped, plain], dp_std=0.5)
    with pytest.raises(ValueError, match="dp_clip on every bucket"):
        FedAvgExchange([plain], dp_std=0.5)
    weighted = FedAvgBucket(global_engine(), kernels=K, dp_clip=1.0, weight=2.0)
    with pytest.raises(ValueError, match="client weight"):
        FedAvgExchange([weighted], dp_std=0.5)
    robust = FedAvgBucket(global_engine(), kernels=K, dp_clip=1.0, robust="median")
    with pytest.raises(ValueError, match="robust"):
        FedAvgExchange([robust], robust="median", dp_std=0.5)
    for bad_std in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="dp_std"):
            FedAvgExchange([clipped], dp_std=bad_std)
    for bad_seed in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="dp_seed"):
            FedAvgExchange([clipped], dp_std=0.5, dp_seed=bad_seed)
    FedAvgExchange([weighted])                    # clipping alone combines with weights ...
    FedAvgExchange([robust], robust="median")     # ... and with the robust aggregation
    assert FedAvgExchange([clipped], dp_std=0.5, dp_seed=7).state_dict() == {"round": 0, "seed": 7}
    # without dp_clip the host kernels of the other test files (no DP attributes) still serve
    assert FedAvgBucket(global_engine(), kernels=HostKernels).run() == 1
    assert plain.clip_stats()[1] == 1.0 and math.isnan(plain.clip_stats()[0])


def test_config_keys_and_trainer_validation(tmp_path, capsys):
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    from federated_multi_modal_amd.trainers import MaPLeFederated
    cfg = get_cfg_default()
    extend_cfg(cfg)
    assert (cfg.FED.DP_CLIP, cfg.FED.DP_NOISE_MULTIPLIER, cfg.FED.DP_DELTA, cfg.FED.DP_SEED) == (0.0, 0.0, 1e-5, -1)
    cfg.merge_from_list(["FED.DP_CLIP", "1e30", "FED.DP_NOISE_MULTIPLIER", 1, "FED.DP_DELTA", "1e-6",
                         "FED.DP_SEED", 42])
    assert (cfg.FED.DP_CLIP, cfg.FED.DP_NOISE_MULTIPLIER, cfg.FED.DP_DELTA, cfg.FED.DP_SEED) == (1e30, 1.0, 1e-6, 42)
    yaml = tmp_path / "dp.yaml"
    yaml.write_text("FED:\n  DP_CLIP: 0.25\n  DP_NOISE_MULTIPLIER: 1.5\n  DP_DELTA: 0.001\n  DP_SEED: 9\n")
    cfg2 = get_cfg_default()
    extend_cfg(cfg2)
    cfg2.merge_from_file(str(yaml))
    assert (cfg2.FED.DP_CLIP, cfg2.FED.DP_NOISE_MULTIPLIER, cfg2.FED.DP_DELTA, cfg2.FED.DP_SEED) == (0.25, 1.5, 1e-3, 9)
    with pytest.raises(ValueError):
        cfg2.merge_from_list(["FED.DP_CLIP", "much"])

    def check(rank=0, seed=3, **keys):
        tr = MaPLeFederated.__new__(MaPLeFederated)
        tr.num_clients, tr.rank = 4, rank
        tr.cfg = get_cfg_default()
        tr.cfg.SEED = seed
        fed = {"DP_CLIP": 0.0, "DP_NOISE_MULTIPLIER": 0.0, "DP_DELTA": 1e-5, "DP_SEED": -1, "ROBUST_AGG": "none",
               "CLIENT_WEIGHTS": "uniform"}
        fed.update(keys)
        return tr._dp_cfg(fed.get)

    assert check() == {"clip": None, "z": 0.0, "std": 0.0, "delta": 1e-5, "seed": 3}
    assert capsys.readouterr().out == ""
    assert check(seed=-1)["seed"] == 0 and check(DP_SEED=11)["seed"] == 11
    got = check(DP_CLIP=0.3, DP_NOISE_MULTIPLIER=1.1)
    assert got["clip"] == 0.3 and got["std"] == float(np.float32(1.1) * np.float32(0.3))
    out = capsys.readouterr().out
    assert "[INFO] DP-FedAvg" in out and "eps" in out
    check(DP_CLIP=0.3, rank=1)
    assert capsys.readouterr().out == ""  # rank 0 alone reports
    # the clipping half alone combines with the other options
    assert check(DP_CLIP=2.0, ROBUST_AGG="median")["clip"] == 2.0
    assert check(DP_CLIP=2.0, CLIENT_WEIGHTS="samples")["clip"] == 2.0
    for key, keys in (("FED.DP_CLIP", dict(DP_CLIP=-1.0)),
                      ("FED.DP_CLIP", dict(DP_CLIP=float("inf"))),
                      ("FED.DP_CLIP", dict(DP_CLIP="1")),
                      ("FED.DP_NOISE_MULTIPLIER", dict(DP_CLIP=1.0, DP_NOISE_MULTIPLIER=-0.5)),
                      ("FED.DP_NOISE_MULTIPLIER", dict(DP_CLIP=1.0, DP_NOISE_MULTIPLIER=float("nan"))),
                      ("FED.DP_CLIP", dict(DP_NOISE_MULTIPLIER=1.0)),                    # noise without a bound
                      ("FED.CLIENT_WEIGHTS", dict(DP_CLIP=1.0, DP_NOISE_MULTIPLIER=1.0, CLIENT_WEIGHTS="samples")),
                      ("FED.CLIENT_WEIGHTS", dict(DP_CLIP=1.0, DP_NOISE_MULTIPLIER=1.0, CLIENT_WEIGHTS=(1, 2, 3, 4))),
                      ("FED.ROBUST_AGG", dict(DP_CLIP=1.0, DP_NOISE_MULTIPLIER=1.0, ROBUST_AGG="median")),
                      ("FED.DP_DELTA", dict(DP_DELTA=0.0)),
                      ("FED.DP_DELTA", dict(DP_DELTA=1.0)),
                      ("FED.DP_DELTA", dict(DP_DELTA=-0.1)),
                      ("FED.DP_SEED", dict(DP_SEED=-2)),
                      ("FED.DP_SEED", dict(DP_SEED=1.5))):
        with pytest.raises(ValueError, match=key):
            check(**keys)


def test_abi_argument_checks_run_before_any_launch():
    """The three entry points' error returns, on the host: no device is touched."""
    from federated_multi_modal_amd import _lib, ops
    F = 4  # any non-null address: every call below returns before it is read
    for name, args, text in (
            ("mf_dp_update_scale", (F, F, -1, F, F, 8, 1.0, F, F, None), "negative"),
            ("mf_dp_update_scale", (F, F, 8, F, F, 8, 0.0, F, F, None), "clip"),
            ("mf_dp_update_scale", (F, F, 8, F, F, 8, float("nan"), F, F, None), "clip"),
            ("mf_dp_update_scale", (F, F, 8, F, F, 8, 1.0, None, F, None), "workspace"),
            ("mf_dp_update_scale", (F, None, 8, F, F, 8, 1.0, F, F, None), "global copy"),
            ("mf_fedavg_pack_clipped", (F, -1, F, 8, F, F, None, F, 1.0, 0, F, None), "negative"),
            ("mf_fedavg_pack_clipped", (F, 8, F, 8, F, F, None, F, 1.0, 3, F, None), "layout"),
            ("mf_fedavg_pack_clipped", (F, 8, F, 8, F, F, None, F, 0.0, 1, F, None), "weight"),
            ("mf_fedavg_pack_clipped", (F, 8, F, 8, F, F, None, None, 1.0, 0, F, None), "scale"),
            ("mf_fedavg_pack_clipped", (F, 8, F, 8, None, F, None, F, 1.0, 0, F, None), "global copy"),
            ("mf_dp_add_noise", (F, -1, 0, 1, 0, 1.0, None), "negative"),
            ("mf_dp_add_noise", (F, 8, -4, 1, 0, 1.0, None), "negative"),
            ("mf_dp_add_noise", (F, 8, 2 ** 63 - 4, 1, 0, 1.0, None), "overflow"),
            ("mf_dp_add_noise", (F, 8, 0, 1, 0, -1.0, None), "std"),
            ("mf_dp_add_noise", (F, 8, 0, 1, 0, float("inf"), None), "std"),
            ("mf_dp_add_noise", (None, 8, 0, 1, 0, 1.0, None), "null")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call(name, *args)
    assert _lib.call("mf_dp_add_noise", F, 0, 0, 1, 0, 1.0, None) == 0    # nothing to do
    assert _lib.call("mf_dp_add_noise", F, 8, 0, 1, 0, 0.0, None) == 0    # std 0: no launch, the bits stay
    assert ops.dp_update_ws_floats(37, 4099) == 2 and ops.dp_update_ws_floats(8200, 8) == 3
    assert ops.dp_update_ws_floats(0, 0) == 1 and ops.dp_update_ws_floats(8192, 0) == 1
    p16, p32 = torch.zeros(8, dtype=torch.float16), torch.zeros(8)
    g16, g32, ws, out = p16.clone(), p32.clone(), torch.zeros(2), torch.zeros(3)
    for kw, text in ((dict(clip=0.0), "clip"), (dict(g16=g16[:4]), "g16"), (dict(g32=g32.double()), "g32"),
                     (dict(ws=ws[:0]), "ws"), (dict(out=torch.zeros(2)), "out"), (dict(out=p32[:3]), "overlaps")):
        a = dict(p16=p16, g16=g16, p32=p32, g32=g32, clip=1.0, ws=ws, out=out)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.dp_update_scale(**a)
    bucket, flag, shared = torch.zeros(17), torch.zeros(1, dtype=torch.int32), torch.zeros(32)
    for kw, text in ((dict(layout="median"), "layout"), (dict(layout="weighted", weight=0.0), "weight"),
                     (dict(layout="weighted"), "bucket"), (dict(bucket=bucket[:16]), "bucket"),
                     (dict(scale=None), "scale"), (dict(p32=shared[:8], bucket=shared[:17]), "overlaps")):
        a = dict(p16=p16, p32=p32, g16=g16, g32=g32, invalid_flag=flag, scale=out[1:2], weight=1.0, layout="plain",
                 bucket=bucket)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.fedavg_pack_clipped(**a)
    buf = torch.zeros(8)
    for kw, text in ((dict(buf=buf.double()), "buf"), (dict(offset=-1), "offset"), (dict(seed=-1), "seed"),
                     (dict(seed=2 ** 64), "seed"), (dict(round_=2 ** 32), "round"), (dict(std=-1.0), "std"),
                     (dict(std=float("nan")), "std")):
        a = dict(buf=buf, offset=0, seed=1, round_=0, std=1.0)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.dp_add_noise(**a)
