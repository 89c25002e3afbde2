"""CPU tier: int8 compression of the FedAvg uplink with error feedback (FedAvgBucket compress="int8"; FED.COMPRESS)
through the collective protocol of federated_multi_modal_amd/federated.py on gloo ranks, with a host restatement of
mf_compress_quantize / mf_compress_decode in numpy fp32 (CompressHostKernels) in the kernels' place.  The GPU tier,
tests/test_fedavg_compress_gpu.py, checks the kernels against the same restatement.

The arithmetic is fully specified (include/mapfed.h): every comparison here is bit for bit."""
import math

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_fedavg_dist import FakeEngine, HostKernels, _init, _spawn
from test_fedavg_dp_dist import MASK, DPHostKernels, philox4x32_10
from test_fedavg_robust_dist import MEDIAN_TRIM, QNAN_BITS, host_trimmed
from test_fedopt_dist import HP, FedOptHostKernels, _f, host_step

B = 256
N16, N32 = 37, 4096 + 3
N = N16 + N32
SEED = 0x0FED_C0DE_1234_5678  # both key words in use
F32 = np.float32


# ----------------------------------------------------------------------------- the restatement

def host_rand(i, seed, rnd, client):
    """r_i = float(w >> 8) * 2^-24 in [0, 1): w = word i & 3 of Philox4x32-10 on the counter
    (i >> 2 low, i >> 2 high, round, 0x80000000 | client) under the key seed."""
    i = np.asarray(i, dtype=np.uint64)
    q, lane = i >> np.uint64(2), (i & np.uint64(3)).astype(np.int64)
    x = philox4x32_10(q & MASK, q >> np.uint64(32), np.full_like(q, rnd), np.full_like(q, 0x80000000 | client),
                      seed & MASK, seed >> 32)
    w = np.choose(lane, x)
    return (w >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)


def host_quantize(x, g, e, bad, rounding, seed, rnd, client, padded):
    """x, g: the n fp32 values float(x_i), float(g_i); e: the fp32 residual or None.  Returns (int8 codes [padded],
    fp32 scales [padded / 256], e' or None), every step one fp32 operation."""
    x, g = np.asarray(x, dtype=F32), np.asarray(g, dtype=F32)
    n = x.size
    assert padded % B == 0 and padded >= n
    if bad:
        return np.zeros(padded, np.int8), np.zeros(padded // B, F32), None if e is None else e.copy()
    d = x - g
    u = d if e is None else d + np.asarray(e, dtype=F32)
    assert u.dtype == F32
    up = np.zeros(padded, F32)
    up[:n] = u
    blocks = up.reshape(-1, B)
    amax = np.fmax.reduce(np.abs(blocks), axis=1)
    scale = amax / F32(127.0)
    with np.errstate(all="ignore"):
        t = blocks / scale[:, None]
        f = np.floor(t)
        if rounding == "nearest":
            q = np.rint(t)
        else:
            assert rounding == "stochastic"
            p = t - f
            r = host_rand(np.arange(padded, dtype=np.uint64), seed, rnd, client).reshape(-1, B)
            q = f + (r < p).astype(F32)
        q = np.fmin(np.fmax(q, F32(-127.0)), F32(127.0))
        zero = amax == 0
        q[zero] = 0
        sq = scale[:, None] * q
        en = blocks - sq
        en[zero] = blocks[zero]
    assert q.dtype == F32 and en.dtype == F32
    return q.astype(np.int8).reshape(-1), scale, None if e is None else en.reshape(-1)[:n].copy()


def host_dequant(g, codes, scales):
    """y_i = g_i + scale * q, one fp32 multiply and one fp32 add, for i < n."""
    g = np.asarray(g, dtype=F32)
    sq = np.repeat(np.asarray(scales, dtype=F32), B)[:g.size] * codes[:g.size].astype(F32)
    return g + sq


def chunk_bytes(S):
    assert S > 0 and S % B == 0
    return S + S // 64 + 8


def _cat(a16, a32):
    return torch.cat([a16.float(), a32]).numpy()


class CompressHostKernels(DPHostKernels):
    """The host kernels plus the compression three, with the signatures of ops.compress_chunk_bytes,
    ops.compress_quantize and ops.compress_decode."""

    @staticmethod
    def compress_chunk_bytes(S):
        return chunk_bytes(S)

    @staticmethod
    def compress_quantize(p16, p32, g16, g32, e_in, e_out, invalid, weight, rounding, seed, rnd, client, image, slot, S):
        world, C, chunk = image.shape
        assert image.dtype == torch.uint8 and chunk == chunk_bytes(S) and (e_in is None) == (e_out is None)
        bad = bool(invalid.item())
        codes, scales, en = host_quantize(_cat(p16, p32), _cat(g16, g32), None if e_in is None else e_in.numpy(), bad,
                                          rounding, seed, rnd, client, world * S)
        if e_out is not None:
            assert e_out.data_ptr() != e_in.data_ptr()
            e_out.copy_(torch.from_numpy(en))
        tail = np.array([0.0, 0.0] if bad else [1.0 if weight is None else weight, 1.0], dtype=F32)
        for r in range(world):
            raw = np.concatenate([codes[r * S:(r + 1) * S].view(np.uint8), scales[r * S // B:(r + 1) * S // B].view(np.uint8),
                                  tail.view(np.uint8)])
            image[r, slot].copy_(torch.from_numpy(raw))

    @staticmethod
    def compress_decode(image, nclients, chunk_stride, S, first, first_step, g16, g32, layout, out, out_stride):
        raw = image.numpy()
        g = _cat(g16, g32)
        n = g.size
        for c in range(nclients):
            ch = raw[c * chunk_stride:c * chunk_stride + chunk_bytes(S)]
            codes, scales = ch[:S].view(np.int8), ch[S:S + S // 64].view(F32)
            w, vote = ch[S + S // 64:].view(F32)
            i = first + c * first_step + np.arange(S)
            if vote == 0:
                y = np.full(S, QNAN_BITS, np.int32).view(F32) if layout == "robust" else np.zeros(S, F32)
            else:
                gi = np.where(i < n, g[np.minimum(i, n - 1)], F32(0))
                yy = gi + np.repeat(scales, B) * codes.astype(F32)
                y = np.where(i < n, w * yy if layout == "weighted" else yy, F32(0)).astype(F32)
                y[i == n] = vote if layout == "plain" else w
                if layout != "plain":
                    y[i == n + 1] = vote
            out[c * out_stride:c * out_stride + S].copy_(torch.from_numpy(y))


class CompressFedOptKernels(CompressHostKernels, FedOptHostKernels):
    """... with the server step."""


# ----------------------------------------------------------------------------- every layout, one set of bits

def global_engine():
    return FakeEngine(0, n16=N16, n32=N32)


def local_result(c, rnd, g16, g32, bad=False):
    """Client c's weights after its local training of round rnd, from the global weights it was given."""
    g = torch.Generator().manual_seed(900 + 10 * rnd + c)
    p16 = (g16.float() + 1e-2 * torch.randn(N16, generator=g)).half()
    p32 = g32 + 1e-3 * torch.randn(N32, generator=g) * (1.0 + g32.abs())
    if bad:
        p32[3] = float("nan")
    return p16, p32


def scenarios(n):
    """name -> per round (invalid clients, clients that fail after they were packed)."""
    return {"clean": (((), ()), ((), ())), "bad": (((1,), ()), ((), ())), "late": (((), (n - 1,)), ((), ())),
            "nobody": (((), ()), (tuple(range(n)), ()))}


def padded_for(world, tail):
    return -(-(N + tail) // (world * B)) * world * B


def expected(n, scen, rounding="stochastic", error_feedback=True, weights=None, robust=None, server=None, world=1):
    """One process, no exchange: two rounds in numpy / torch fp32.  Returns ([n_valid per round], flat16, flat32,
    [residual per client])."""
    ge = global_engine()
    g16, g32 = ge.flat16.clone(), ge.flat32.clone()
    tail = 1 if weights is None and robust is None else 2
    res = [np.zeros(N, F32) if error_feedback else None for _ in range(n)]
    if server is not None:
        sx = torch.cat([g16.float(), g32])
        sm, sv = torch.zeros_like(sx), torch.full_like(sx, float(_f(HP["tau"]) * _f(HP["tau"])))
    valid = []
    for rnd, (bad, late) in enumerate(scen):
        g = _cat(g16, g32)
        rows, ws = [], []
        for c in range(n):
            p16, p32 = local_result(c, rnd, g16, g32, c in bad)
            out = c in bad or c in late
            codes, scales, en = host_quantize(_cat(p16, p32), g, res[c], out, rounding, SEED, rnd, c,
                                              padded_for(world, tail))
            if error_feedback:
                if out:
                    assert np.array_equal(en.view(np.int32), res[c].view(np.int32))  # untouched
                res[c] = en
            if not out:
                rows.append(torch.from_numpy(host_dequant(g, codes, scales)))
                ws.append(torch.tensor(1.0 if weights is None else weights[c], dtype=torch.float32))
        valid.append(len(rows))
        if not rows:
            continue
        if robust is not None:
            stat = host_trimmed(torch.stack(rows), MEDIAN_TRIM if robust == "median" else 1)
            div = torch.tensor(1.0)
        else:
            acc = div = None
            for y, w in zip(rows, ws):
                term = y * w if weights is not None else y
                acc = term if acc is None else acc + term
                div = w.clone() if div is None else div + w
            stat = acc
        if server is not None:
            sx, sm, sv = host_step(server, stat, div, sx, sm, sv, **HP)
            v = sx.half()
        else:
            v = (stat / div).half()
        g16, g32 = v[:N16].clone(), v[N16:].float()
    return valid, g16, g32, res


def run_rounds(ids, scen, rounding="stochastic", error_feedback=True, weights=None, robust=None, server=None,
               kernels="host", device=None, **bkw):
    """The same two rounds through FedAvgBucket / FedAvgExchange for the clients `ids` of this process.  kernels: the
    host restatement, or None for the bucket's default (the device kernels; the GPU tier)."""
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange, ServerOptimizer
    if kernels == "host":
        kernels = CompressFedOptKernels if server is not None else CompressHostKernels
    engines = [global_engine() for _ in ids]
    if device is not None:
        for e in engines:
            e.device, e.flat16, e.flat32 = device, e.flat16.to(device), e.flat32.to(device)
    kw = dict(bkw) if kernels is None else dict(bkw, kernels=kernels)
    sv = None if server is None else ServerOptimizer(server, engines[0], **HP)
    feds = [FedAvgBucket(e, compress="int8", compress_rounding=rounding, error_feedback=error_feedback,
                         compress_seed=SEED, client=c, weight=None if weights is None else weights[c], robust=robust,
                         server=sv, **kw) for e, c in zip(engines, ids)]
    x = FedAvgExchange(feds, robust=robust, **{k: v for k, v in bkw.items() if k in ("mode", "shard_single")})
    valid = []
    for rnd, (bad, late) in enumerate(scen):
        for e, c in zip(engines, ids):
            p16, p32 = local_result(c, rnd, e.flat16.cpu(), e.flat32.cpu(), c in bad)
            e.flat16.copy_(p16)
            e.flat32.copy_(p32)
        for f in feds:
            f.pack()
        x.start()
        x.finish([j for j, c in enumerate(ids) if c in late])
        assert x.round == rnd + 1
        valid.append(x.n_valid())
        for f in feds:
            f.unpack()
    return valid, [(e.flat16.cpu().clone(), e.flat32.cpu().clone(), None if f.resid is None else f.resid.cpu().clone())
                   for e, f in zip(engines, feds)]


def check(got, want, where):
    valid, clients = got
    ref_valid, ref16, ref32, res = want
    assert valid == ref_valid, where
    for c, (p16, p32, e) in clients:
        assert torch.equal(p16, ref16) and torch.equal(p32, ref32), (where, c)
        if res[c] is None:
            assert e is None
        else:
            assert np.array_equal(e.numpy().view(np.int32), res[c].view(np.int32)), (where, c)


# (name, run_rounds / expected keywords); the first four run at every layout, the rest at 2 x 2 and in one process
VARIANTS = [("nearest", dict(rounding="nearest")), ("no_feedback", dict(error_feedback=False)),
            ("weighted", dict(weights=(3.0, 1.0, 2.0, 0.5, 1.5, 4.0, 1.0, 2.0))), ("median", dict(robust="median")),
            ("trimmed", dict(robust="trimmed_mean")), ("fedadam", dict(server="fedadam")),
            ("weighted_fedavgm", dict(weights=(3.0, 1.0, 2.0, 0.5, 1.5, 4.0, 1.0, 2.0), server="fedavgm"))]


def cases(n, which):
    if which == "allreduce":
        return [(name, scen, {"mode": "allreduce"}) for name, scen in scenarios(n).items()]
    out = [(name, scen, {}) for name, scen in scenarios(n).items()]
    if which == "variants":
        out += [(name, scenarios(n)["bad"], kw) for name, kw in VARIANTS]
    return out


def _worker(rank, world, port, per_rank, variants, out):
    _init(rank, world, port)
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    out[rank] = {name: run_rounds(ids, scen, **kw) for name, scen, kw in cases(world * per_rank, variants)}
    dist.destroy_process_group()


@pytest.mark.parametrize("world,per_rank", [(2, 1), (3, 1), (8, 1), (2, 2), (3, 2)])
def test_compressed_exchange_is_bit_exact_at_every_layout(world, per_rank):
    """Two consecutive rounds (the residual carries over), stochastic rounding: clean, an invalid client, a late
    failure and nobody valid.  Every layout ends with the restatement's fp16 weights, residuals and n_valid bit for
    bit, and so does the same client set in one process.  At world 3 a shard is 6 blocks, no multiple of 4.  At 2 x 2
    also: nearest rounding, no error feedback, client weights, the median, the trimmed mean and a server optimizer."""
    n = world * per_rank
    if world == 3:
        assert (padded_for(3, 1) // 3 // B) % 4 != 0
    variants = "variants" if (world, per_rank) == (2, 2) else "plain"
    res = _spawn(_worker, world, per_rank, variants)
    for name, scen, kw in cases(n, variants):
        want = expected(n, scen, world=world, **kw)
        assert want[0][-1] == (0 if name == "nobody" else n) and want[0][0] == n - (name in ("bad", "late") or bool(kw))
        for r in range(world):
            ids = range(r * per_rank, (r + 1) * per_rank)
            check((res[r][name][0], list(zip(ids, res[r][name][1]))), want, (name, r))
        one = run_rounds(list(range(n)), scen, **kw)
        check((one[0], list(enumerate(one[1]))), expected(n, scen, world=1, **kw), (name, "one process"))
        if kw.get("error_feedback", True):
            assert any(e.any() for e in want[3])
        if name == "nobody":  # round 1 kept round 0's global weights, and every residual
            first = expected(n, scen[:1], world=world)
            assert torch.equal(want[1], first[1]) and torch.equal(want[2], first[2])
            assert all(np.array_equal(a, b) for a, b in zip(want[3], first[3]))


@pytest.mark.parametrize("name,kw", VARIANTS)
def test_layouts_and_combinations_in_one_process(name, kw):
    """Three clients, one of them invalid in round 0: plain with nearest rounding and without error feedback, the
    weighted and the robust layouts, and a server optimizer on the plain and on the weighted mean."""
    scen = scenarios(3)["bad"]
    one = run_rounds([0, 1, 2], scen, **kw)
    check((one[0], list(enumerate(one[1]))), expected(3, scen, **kw), name)


def test_allreduce_mode_decodes_locally():
    """"allreduce" decodes every bucket locally and then sums as before (no traffic is saved).  Two ranks, where the
    all_reduce's order cannot differ from the client order (a + b), so the bits are the restatement's."""
    res = _spawn(_worker, 2, 1, "allreduce")
    for name, scen, kw in cases(2, "allreduce"):
        want = expected(2, scen, world=2)
        for r in range(2):
            check((res[r][name][0], [(r, res[r][name][1][0])]), want, (name, r))


# ----------------------------------------------------------------------------- residual handling

def _three(rounding="stochastic", **kw):
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    engines = [global_engine() for _ in range(3)]
    feds = [FedAvgBucket(e, kernels=CompressHostKernels, compress="int8", compress_rounding=rounding,
                         compress_seed=SEED, client=c, **kw) for c, e in enumerate(engines)]
    return engines, feds, FedAvgExchange(feds)


def _train(engines, rnd, bad=()):
    for c, e in enumerate(engines):
        p16, p32 = local_result(c, rnd, e.flat16, e.flat32, c in bad)
        e.flat16.copy_(p16)
        e.flat32.copy_(p32)


def test_late_failure_repack_gives_the_same_codes_and_commits_once():
    engines, feds, x = _three()
    for rnd in range(2):
        _train(engines, rnd)
        before = [f.resid.clone() for f in feds]
        for f in feds:
            f.pack()
        first = x.image.clone()
        assert all(torch.equal(f.resid, b) for f, b in zip(feds, before))  # pack writes e', not e
        x.start()
        x.finish([2])  # client 2 failed after it was packed: every local bucket packs again
        assert x.round == rnd + 1
        assert torch.equal(x.image[:, :2], first[:, :2])      # the same codes, scales and tails
        assert not x.image[:, 2].any() and first[:, 2].any()  # the failed client now sends nothing
        want = [f.resid_next.clone() for f in feds]
        for f in feds:
            f.unpack()
        assert x.n_valid() == 2
        for c, f in enumerate(feds):
            assert torch.equal(f.resid, before[c] if c == 2 else want[c]), c
        assert not feds[2].resid.any() and feds[0].resid.any()
        kept = [f.resid.clone() for f in feds]
        for f in feds:
            f.unpack()  # a second unpack of the same round commits nothing
        assert all(torch.equal(f.resid, k) for f, k in zip(feds, kept))


def test_failed_and_invalid_clients_keep_their_residual():
    engines, feds, x = _three()
    _train(engines, 0)
    for f in feds:
        f.pack()
    x.start()
    x.finish()
    for f in feds:
        f.unpack()
    kept = [f.resid.clone() for f in feds]
    assert all(k.any() for k in kept)
    _train(engines, 1, bad=(1,))
    feds[0].pack(failed=True)
    feds[1].pack()
    feds[2].pack()
    x.start()
    x.finish()
    for f in feds:
        f.unpack()
    assert x.n_valid() == 1
    assert torch.equal(feds[0].resid, kept[0]) and torch.equal(feds[1].resid, kept[1])
    assert not torch.equal(feds[2].resid, kept[2])


def test_residual_state_dict_round_trips(tmp_path):
    engines, feds, x = _three()
    _train(engines, 0)
    for f in feds:
        f.pack()
    x.start()
    x.finish()
    for f in feds:
        f.unpack()
    sd = feds[0].state_dict()
    assert sd["residual"].dtype == torch.float32 and sd["residual"].device.type == "cpu" and sd["residual"].any()
    torch.save(sd, tmp_path / "resid.pt")
    sd = torch.load(tmp_path / "resid.pt", weights_only=True)
    feds = [feds[0]] + _three()[1][1:]  # two fresh buckets beside it
    assert not feds[1].resid.any()
    feds[1].load_state_dict(sd)
    assert torch.equal(feds[1].resid, feds[0].resid) and sd["residual"].data_ptr() != feds[1].resid.data_ptr()
    feds[1].load_state_dict({"residual": None})
    assert not feds[1].resid.any()
    for bad in (torch.zeros(N - 1), torch.zeros(N, dtype=torch.float64), [0.0] * N):
        with pytest.raises(ValueError, match="residual"):
            feds[1].load_state_dict({"residual": bad})
    _, plain, _ = _three(error_feedback=False)
    assert plain[0].state_dict() == {"residual": None}
    with pytest.raises(ValueError, match="residual"):
        plain[0].load_state_dict(sd)


# ----------------------------------------------------------------------------- quantisation properties

def test_no_error_feedback_allocates_no_residual():
    engines, feds, x = _three(error_feedback=False)
    assert all(f.resid is None and f.resid_next is None for f in feds)
    _train(engines, 0)
    for f in feds:
        f.pack()
    x.start()
    x.finish()
    for f in feds:
        f.unpack()
    assert x.n_valid() == 3 and all(f.resid is None and f.resid_next is None for f in feds)


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_all_zero_update_gives_zero_scales_and_the_global_weights(rounding):
    engines, feds, x = _three(rounding)
    for f in feds:
        f.pack()
    S = x.S
    img = x.image.numpy()
    assert not img[:, :, :S + S // 64].any()                                  # codes and scales
    assert (img[:, :, S + S // 64:].view(F32) == 1.0).all()                   # weight 1, vote 1
    g = global_engine()
    gcat = torch.cat([g.flat16.float(), g.flat32])
    x.decode_local()
    for f in feds:  # g + 0 * 0: the weights g themselves, and the vote
        assert torch.equal(f.buf[:N].view(torch.int32), gcat.view(torch.int32)) and f.buf[N] == 1.0
        assert not f.pbuf[N + 1:].any()
    x.start()
    x.finish()
    want = ((gcat + gcat + gcat) / 3.0).half()
    for f, e in zip(feds, engines):
        f.unpack()
        assert torch.equal(e.flat16, g.flat16) and torch.equal(e.flat16, want[:N16])
        assert torch.equal(e.flat32, want[N16:].float())
        assert not f.resid.any()


def _sample_update(n, seed):
    g = np.random.default_rng(seed)
    u = (g.standard_normal(n) * np.exp2(g.integers(-8, 3, n))).astype(F32)
    u[B:2 * B] = 0                      # an all-zero block
    u[2 * B:3 * B] *= F32(1e-3)
    u[2 * B + 5] = F32(-7.0)            # one large value: t = -127 there, everything else rounds to 0 or +-1
    return u


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_residual_bound(rounding):
    """|e'| <= scale / 2 (nearest) or scale (stochastic), times 1 + 2^-22 for the roundings of t, scale * q and the
    subtraction; the codes stay inside [-127, 127] and reach both ends."""
    n = 40 * B + 17
    u = _sample_update(n, 1)
    padded = 41 * B
    codes, scales, en = host_quantize(u, np.zeros(n, F32), np.zeros(n, F32), False, rounding, SEED, 3, 2, padded)
    s = np.repeat(scales, B)[:n].astype(np.float64)
    bound = s * (0.5 if rounding == "nearest" else 1.0) * (1.0 + 2.0 ** -22)
    assert (np.abs(en.astype(np.float64)) <= bound).all()
    assert codes.min() == -127 and codes.max() == 127 and not codes[B:2 * B].any() and scales[1] == 0
    assert codes[2 * B + 5] == -127 and np.abs(codes[2 * B:3 * B]).sum() <= 127 + B
    assert not codes[n:].any()
    # u = scale * q + e' up to the rounding of the product and of the difference
    assert np.abs(s * codes[:n] + en - u).max() <= 2.0 ** -23 * np.abs(u).max()


def test_stochastic_rounding_is_unbiased():
    """A fixed u over 2^16 coordinates, 64 rounds: per coordinate Var(scale * q) = scale^2 p (1 - p) <= scale^2 / 4, so
    the mean of scale * q - u over the 2^22 samples has a standard deviation of at most scale / (2 sqrt(2^22)), scale
    the largest block scale; it must lie within 5 sigma of 0.  (The rounding of t = u / scale moves p by 127 * 2^-24
    at most, a bias of 7.6e-6 scale against the 1.2e-3 scale allowed.)  Nearest rounding of the same u is biased far
    beyond that when u sits off-centre between two codes."""
    n = 1 << 16
    u = _sample_update(n, 2)
    zeros = np.zeros(n, F32)
    tot = np.zeros(n, np.float64)
    for rnd in range(64):
        codes, scales, _ = host_quantize(u, zeros, None, False, "stochastic", SEED, rnd, 5, n)
        tot += np.repeat(scales, B).astype(np.float64) * codes
    mean = (tot / 64 - u).mean()
    sigma = float(scales.max()) / (2.0 * math.sqrt(2.0 ** 22))
    print(f"stochastic rounding: mean error {mean:.3e}, sigma {sigma:.3e}, largest scale {scales.max():.3e}")
    assert abs(mean) <= 5.0 * sigma
    # off-centre values, one scale: nearest rounds every one of them the same way
    v = np.full(n, 0.3, F32)
    v[::B] = 127.0
    cn, sn, _ = host_quantize(v, zeros, None, False, "nearest", SEED, 0, 5, n)
    assert abs((np.repeat(sn, B).astype(np.float64) * cn - v).mean()) > 5.0 * float(sn.max()) / (2.0 * math.sqrt(n))
    tot[:] = 0
    for rnd in range(64):
        cs, ss, _ = host_quantize(v, zeros, None, False, "stochastic", SEED, rnd, 5, n)
        tot += np.repeat(ss, B).astype(np.float64) * cs
    assert abs((tot / 64 - v).mean()) <= 5.0 * float(ss.max()) / (2.0 * math.sqrt(2.0 ** 22))


def test_rounding_bits_depend_on_seed_round_client_and_coordinate_alone():
    """The same update quantised for one destination rank and for three (other shard lengths, other chunks) gives
    the same codes and scales; another round, client or seed gives other codes."""
    i = np.arange(5000, dtype=np.uint64)
    r = host_rand(i, SEED, 3, 2)
    assert np.array_equal(r[1237:2001], host_rand(i[1237:2001], SEED, 3, 2))
    assert r.min() >= 0.0 and r.max() < 1.0
    for other in ((SEED + 1, 3, 2), (SEED + 2 ** 32, 3, 2), (SEED, 4, 2), (SEED, 3, 1)):
        assert not np.array_equal(r, host_rand(i, *other))
    # disjoint from the noise streams: the counter's last word
    noise = philox4x32_10(i >> np.uint64(2), np.zeros_like(i), np.full_like(i, 3), np.zeros_like(i), SEED & MASK,
                          SEED >> 32)
    assert not np.array_equal((np.choose((i & np.uint64(3)).astype(np.int64), noise) >> np.uint64(8)).astype(F32)
                              * F32(2.0 ** -24), host_rand(i, SEED, 3, 0))
    e = global_engine()
    p16, p32 = local_result(1, 0, e.flat16, e.flat32)
    flag = torch.zeros(1, dtype=torch.int32)
    padded = padded_for(3, 1)
    assert padded == padded_for(1, 1) + B  # 4608 for three ranks, 4352 for one

    def image(world, total, rnd=7, client=1, seed=SEED):
        S = total // world
        img = torch.zeros(world, 1, chunk_bytes(S), dtype=torch.uint8)
        CompressHostKernels.compress_quantize(p16, p32, e.flat16, e.flat32, None, None, flag, None, "stochastic", seed,
                                              rnd, client, img, 0, S)
        raw = img.numpy()[:, 0]
        return (np.concatenate([raw[r, :S] for r in range(world)]),
                np.concatenate([raw[r, S:S + S // 64] for r in range(world)]))

    codes, scales = image(1, padded)
    for world in (2, 3, 6, 18):
        c, s = image(world, padded)
        assert np.array_equal(c, codes) and np.array_equal(s, scales), world
    assert np.array_equal(image(1, padded_for(1, 1))[0], codes[:padded_for(1, 1)])
    for kw in (dict(rnd=8), dict(client=2), dict(seed=SEED ^ 1)):
        assert not np.array_equal(image(1, padded, **kw)[0], codes)


# ----------------------------------------------------------------------------- construction, config, ABI

def test_construction_errors():
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    K = CompressHostKernels
    with pytest.raises(ValueError, match="compress"):
        FedAvgBucket(global_engine(), kernels=K, compress="int4")
    with pytest.raises(ValueError, match="compress_rounding"):
        FedAvgBucket(global_engine(), kernels=K, compress="int8", compress_rounding="up")
    with pytest.raises(ValueError, match="compress_rounding"):
        FedAvgBucket(global_engine(), kernels=K, compress_rounding="up")
    for bad_seed in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError, match="compress_seed"):
            FedAvgBucket(global_engine(), kernels=K, compress="int8", compress_seed=bad_seed)
    for bad_client in (-1, 2 ** 31, 0.5, True):
        with pytest.raises(ValueError, match="client"):
            FedAvgBucket(global_engine(), kernels=K, compress="int8", client=bad_client)
    with pytest.raises(ValueError, match="dp_clip"):
        FedAvgBucket(global_engine(), kernels=K, compress="int8", dp_clip=1.0)
    a = FedAvgBucket(global_engine(), kernels=K, compress="int8")
    with pytest.raises(ValueError, match="dp_clip"):
        FedAvgExchange([a], dp_std=0.5)
    for other in (dict(), dict(compress="int8", compress_rounding="stochastic", client=1),
                  dict(compress="int8", error_feedback=False), dict(compress="int8", compress_seed=1)):
        b = FedAvgBucket(global_engine(), kernels=K, **other)
        if not other:
            assert b.pbuf.numel() == N + 1 and a.pbuf.numel() == padded_for(1, 1)  # off: the bucket as it was
            with pytest.raises((ValueError, AssertionError)):
                FedAvgExchange([a, b])
            continue
        with pytest.raises(ValueError, match="compression settings"):
            FedAvgExchange([a, b])
    s = [FedAvgBucket(global_engine(), kernels=K, compress="int8", compress_rounding="stochastic") for _ in range(2)]
    with pytest.raises(ValueError, match="client index"):
        FedAvgExchange(s)  # both at client 0: their rounding bits would coincide
    FedAvgExchange([FedAvgBucket(global_engine(), kernels=K, compress="int8") for _ in range(2)])  # nearest: no bits
    # off by default, and the host kernels of the other test files (no compression attributes) still serve
    plain = FedAvgBucket(global_engine(), kernels=HostKernels)
    assert plain.compress is None and plain.resid is None and plain.run() == 1
    assert plain.exchange.image is None and plain.state_dict() == {"residual": None}
    # a bucket used alone creates its exchange before its first pack
    alone = FedAvgBucket(global_engine(), kernels=K, compress="int8", weight=2.0)
    assert alone._x is None
    assert alone.run() == 1 and alone._x.image.shape == (1, 1, chunk_bytes(padded_for(1, 2)))


def test_config_keys_and_trainer_validation(tmp_path, capsys):
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    from federated_multi_modal_amd.trainers import MaPLeFederated
    cfg = get_cfg_default()
    extend_cfg(cfg)
    keys = lambda c: (c.FED.COMPRESS, c.FED.COMPRESS_ROUNDING, c.FED.COMPRESS_ERROR_FEEDBACK, c.FED.COMPRESS_SEED)  # noqa: E731
    assert keys(cfg) == ("none", "nearest", True, -1)
    cfg.merge_from_list(["FED.COMPRESS", "int8", "FED.COMPRESS_ROUNDING", "stochastic", "FED.COMPRESS_ERROR_FEEDBACK",
                         "False", "FED.COMPRESS_SEED", 42])
    assert keys(cfg) == ("int8", "stochastic", False, 42)
    yaml = tmp_path / "c.yaml"
    yaml.write_text("FED:\n  COMPRESS: int8\n  COMPRESS_ROUNDING: stochastic\n  COMPRESS_ERROR_FEEDBACK: false\n"
                    "  COMPRESS_SEED: 9\n")
    cfg2 = get_cfg_default()
    extend_cfg(cfg2)
    cfg2.merge_from_file(str(yaml))
    assert keys(cfg2) == ("int8", "stochastic", False, 9)

    def check(seed=3, **fed_keys):
        tr = MaPLeFederated.__new__(MaPLeFederated)
        tr.num_clients, tr.rank = 4, 0
        tr.cfg = get_cfg_default()
        tr.cfg.SEED = seed
        fed = {"COMPRESS": "none", "COMPRESS_ROUNDING": "nearest", "COMPRESS_ERROR_FEEDBACK": True, "COMPRESS_SEED": -1,
               "DP_CLIP": 0.0}
        fed.update(fed_keys)
        return tr._compress_cfg(fed.get)

    assert check() == {"compress": None, "rounding": "nearest", "error_feedback": True, "seed": 3}
    assert check(seed=-1)["seed"] == 0 and check(COMPRESS_SEED=11)["seed"] == 11
    assert check(COMPRESS="int8", COMPRESS_ROUNDING="stochastic", COMPRESS_ERROR_FEEDBACK=False) == {
        "compress": "int8", "rounding": "stochastic", "error_feedback": False, "seed": 3}
    assert check(DP_CLIP=1.0)["compress"] is None  # clipping alone is no business of this option
    assert capsys.readouterr().out == ""
    for key, fed_keys in (("FED.COMPRESS", dict(COMPRESS="int4")),
                          ("FED.COMPRESS", dict(COMPRESS=8)),
                          ("FED.COMPRESS", dict(COMPRESS="int8", DP_CLIP=1.0)),
                          ("FED.COMPRESS_ROUNDING", dict(COMPRESS_ROUNDING="up")),
                          ("FED.COMPRESS_ROUNDING", dict(COMPRESS="int8", COMPRESS_ROUNDING=1)),
                          ("FED.COMPRESS_ERROR_FEEDBACK", dict(COMPRESS_ERROR_FEEDBACK="yes")),
                          ("FED.COMPRESS_ERROR_FEEDBACK", dict(COMPRESS_ERROR_FEEDBACK=1)),
                          ("FED.COMPRESS_SEED", dict(COMPRESS_SEED=-2)),
                          ("FED.COMPRESS_SEED", dict(COMPRESS_SEED=1.5)),
                          ("FED.COMPRESS_SEED", dict(COMPRESS_SEED=2 ** 64))):
        with pytest.raises(ValueError, match=key):
            check(**fed_keys)


def test_abi_argument_checks_run_before_any_launch():
    """The entry points' error returns, on the host: no device is touched."""
    from federated_multi_modal_amd import _lib, ops
    F = 4  # any non-null, 4-byte aligned address: every call below returns before it is read
    S = 512
    ch = chunk_bytes(S)
    q = dict(x16=F, g16=F, n16=8, x32=F, g32=F, n32=8, e_in=F, e_out=8, flag=F, weight=1.0, rounding=0, seed=1, rnd=0,
             client=0, image=F, stride=ch, S=S, world=1)
    d = dict(image=F, stride=ch, nclients=2, S=S, first=0, step=0, g16=F, n16=8, g32=F, n32=8, layout=0, out=F,
             ostride=S)
    for name, base, change, text in (
            ("mf_compress_quantize", q, dict(image=None), "null image"),
            ("mf_compress_quantize", q, dict(flag=None), "null image or flag"),
            ("mf_compress_quantize", q, dict(x16=None), "null weights"),
            ("mf_compress_quantize", q, dict(g32=None), "global copy"),
            ("mf_compress_quantize", q, dict(e_out=None), "residual"),
            ("mf_compress_quantize", q, dict(e_in=None), "residual"),
            ("mf_compress_quantize", q, dict(e_out=F), "residual"),
            ("mf_compress_quantize", q, dict(S=500), "multiple of 256"),
            ("mf_compress_quantize", q, dict(S=0), "multiple of 256"),
            ("mf_compress_quantize", q, dict(S=-256), "multiple of 256"),
            ("mf_compress_quantize", q, dict(n16=-1), "negative"),
            ("mf_compress_quantize", q, dict(n32=-1), "negative"),
            ("mf_compress_quantize", q, dict(n32=S), "shorter"),
            ("mf_compress_quantize", q, dict(world=0), "world"),
            ("mf_compress_quantize", q, dict(rounding=2), "rounding"),
            ("mf_compress_quantize", q, dict(rounding=-1), "rounding"),
            ("mf_compress_quantize", q, dict(weight=0.0), "weight"),
            ("mf_compress_quantize", q, dict(weight=float("nan")), "weight"),
            ("mf_compress_quantize", q, dict(weight=float("inf")), "weight"),
            ("mf_compress_quantize", q, dict(client=2 ** 31), "client"),
            ("mf_compress_quantize", q, dict(image=6), "misaligned"),
            ("mf_compress_quantize", q, dict(world=2, n32=S, stride=ch - 4), "stride"),
            ("mf_compress_decode", d, dict(image=None), "null"),
            ("mf_compress_decode", d, dict(out=None), "null"),
            ("mf_compress_decode", d, dict(g16=None), "global copy"),
            ("mf_compress_decode", d, dict(S=300), "multiple of 256"),
            ("mf_compress_decode", d, dict(n32=-1), "negative"),
            ("mf_compress_decode", d, dict(first=-1), "negative"),
            ("mf_compress_decode", d, dict(step=-1), "negative"),
            ("mf_compress_decode", d, dict(nclients=0), "nclients"),
            ("mf_compress_decode", d, dict(layout=3), "layout"),
            ("mf_compress_decode", d, dict(layout=-1), "layout"),
            ("mf_compress_decode", d, dict(stride=ch - 4), "stride"),
            ("mf_compress_decode", d, dict(ostride=S - 1), "stride"),
            ("mf_compress_decode", d, dict(image=5), "misaligned")):
        args = dict(base)
        args.update(change)
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call(name, *args.values(), None)  # the stream last
    assert _lib.call("mf_compress_chunk_bytes", 256) == 268 and _lib.call("mf_compress_chunk_bytes", 1536) == 1568
    for bad in (0, -256, 255, 257):
        assert _lib.call("mf_compress_chunk_bytes", bad) == -1
    assert ops.compress_chunk_bytes(512) == ch == 528
    with pytest.raises(ValueError, match="multiple of 256"):
        ops.compress_chunk_bytes(100)
    p16, p32 = torch.zeros(8, dtype=torch.float16), torch.zeros(8)
    g16, g32, flag = p16.clone(), p32.clone(), torch.zeros(1, dtype=torch.int32)
    e_in, e_out, image = torch.zeros(16), torch.zeros(16), torch.zeros(1, 2, ch, dtype=torch.uint8)
    for kw, text in ((dict(rounding="up"), "rounding"), (dict(weight=0.0), "weight"), (dict(seed=-1), "seed"),
                     (dict(round_=2 ** 32), "round"), (dict(client=2 ** 31), "client"), (dict(g16=g16[:4]), "g16"),
                     (dict(S=100), "multiple of 256"), (dict(image=image.float()), "image"),
                     (dict(image=image[:, :, :ch - 4]), "image"), (dict(slot=2), "slot"), (dict(S=256), "image"),
                     (dict(e_out=None), "both"), (dict(e_out=e_in), "overlaps"), (dict(e_in=e_in[:8]), "e_in"),
                     (dict(invalid_flag=None), "invalid_flag"),
                     (dict(p32=torch.zeros(1024), g32=torch.zeros(1024)), "hold fewer")):
        a = dict(p16=p16, p32=p32, g16=g16, g32=g32, e_in=e_in, e_out=e_out, invalid_flag=flag, weight=None,
                 rounding="nearest", seed=1, round_=0, client=0, image=image, slot=0, S=S)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.compress_quantize(**a)
    flat, out = image.view(-1), torch.zeros(2 * S)
    for kw, text in ((dict(layout="median"), "layout"), (dict(S=100), "multiple of 256"), (dict(nclients=0), "nclients"),
                     (dict(first=-1), "first"), (dict(nclients=3), "image"), (dict(out=out[:S]), "out"),
                     (dict(out=out.double()), "out"), (dict(chunk_stride=ch - 4), "chunk_stride"),
                     (dict(out_stride=S - 4), "out_stride"), (dict(g16=g32), "g16")):
        a = dict(image=flat, nclients=2, chunk_stride=ch, S=S, first=0, first_step=0, g16=g16, g32=g32, layout="plain",
                 out=out, out_stride=S)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.compress_decode(**a)
