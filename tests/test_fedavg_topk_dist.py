"""CPU tier: block-wise top-k sparsification of the FedAvg uplink with error feedback (FedAvgBucket compress="topk";
FED.COMPRESS topk) through the collective protocol of federated_multi_modal_amd/federated.py on gloo ranks, with a host
restatement of mf_topk_select / mf_topk_decode in numpy fp32 (TopkHostKernels) in the kernels' place.  The GPU tier,
tests/test_fedavg_topk_gpu.py, checks the kernels against the same restatement.

The arithmetic is fully specified (include/mapfed.h): every comparison here is bit for bit."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_fedavg_compress_dist import (B, F32, N, N16, N32, CompressHostKernels, _cat, check, chunk_bytes, global_engine,
                                       local_result, padded_for, scenarios)
from test_fedavg_dist import HostKernels, _init, _spawn
from test_fedopt_dist import HP, FedOptHostKernels, _f, host_step

K = 8
U32 = np.uint32


# ----------------------------------------------------------------------------- the restatement

def topk_chunk_bytes(S, k):
    assert S > 0 and S % B == 0 and 1 <= k <= 64
    nbk = S // B * k
    return 4 * nbk + (nbk + 3) // 4 * 4 + 8


def select_blocks(blocks, k):
    """blocks: fp32 [nblk, 256].  The k entries per block that come first under (|u| bits descending, index ascending):
    a stable sort on the 39-bit key (mag << 8) | (255 - index), the k largest, in ascending index order.  Returns
    (uint8 indices [nblk, k], fp32 values [nblk, k], the residual blocks: +0 where kept, u elsewhere)."""
    blocks = np.ascontiguousarray(blocks, dtype=F32)
    mag = (blocks.view(U32) & U32(0x7fffffff)).astype(np.uint64)
    key = (mag << np.uint64(8)) | (np.uint64(255) - np.arange(B, dtype=np.uint64))
    idx = np.sort(np.argsort(key, axis=1, kind="stable")[:, B - k:], axis=1)
    vals = np.take_along_axis(blocks, idx, axis=1)
    en = blocks.copy()
    np.put_along_axis(en, idx, F32(0.0), axis=1)
    return idx.astype(np.uint8), vals, en


def host_select(x, g, e, bad, k, padded):
    """x, g: the n fp32 values float(x_i), float(g_i); e: the fp32 residual or None.  Returns (indices [padded / 256, k],
    values [padded / 256, k], e' or None), every step one fp32 operation."""
    x, g = np.asarray(x, dtype=F32), np.asarray(g, dtype=F32)
    n = x.size
    assert padded % B == 0 and padded >= n
    if bad:
        return np.zeros((padded // B, k), np.uint8), np.zeros((padded // B, k), F32), None if e is None else e.copy()
    d = x - g
    u = d if e is None else d + np.asarray(e, dtype=F32)
    assert u.dtype == F32
    up = np.zeros(padded, F32)
    up[:n] = u
    idx, vals, en = select_blocks(up.reshape(-1, B), k)
    return idx, vals, None if e is None else en.reshape(-1)[:n].copy()


def scatter(idx, vals):
    """s [nblk * 256]: the entry's value at a kept coordinate, +0 elsewhere."""
    s = np.zeros((idx.shape[0], B), F32)
    np.put_along_axis(s, idx.astype(np.int64), vals, axis=1)
    return s.reshape(-1)


def host_dense(g, idx, vals):
    """y_i = g_i + s_i, the one fp32 add, for i < n."""
    g = np.asarray(g, dtype=F32)
    return g + scatter(idx, vals)[:g.size]


def wire(idx, vals, weight, vote, world, S, k):
    """The bytes of the `world` chunks, [world][chunk]."""
    nb = S // B
    pad = np.zeros((nb * k + 3) // 4 * 4 - nb * k, np.uint8)
    tail = np.array([weight, vote], dtype=F32).view(np.uint8)
    return np.stack([np.concatenate([np.ascontiguousarray(vals[r * nb:(r + 1) * nb]).reshape(-1).view(np.uint8),
                                     np.ascontiguousarray(idx[r * nb:(r + 1) * nb]).reshape(-1), pad, tail])
                     for r in range(world)])


class TopkHostKernels(CompressHostKernels):
    """The host kernels plus the top-k three, with the signatures of ops.topk_chunk_bytes, ops.topk_select and
    ops.topk_decode."""

    @staticmethod
    def topk_chunk_bytes(S, k):
        return topk_chunk_bytes(S, k)

    @staticmethod
    def topk_select(p16, p32, g16, g32, e_in, e_out, invalid, weight, k, image, slot, S):
        world, C, chunk = image.shape
        assert image.dtype == torch.uint8 and chunk == topk_chunk_bytes(S, k) and (e_in is None) == (e_out is None)
        bad = bool(invalid.item())
        idx, vals, en = host_select(_cat(p16, p32), _cat(g16, g32), None if e_in is None else e_in.numpy(), bad, k,
                                    world * S)
        if e_out is not None:
            assert e_out.data_ptr() != e_in.data_ptr()
            e_out.copy_(torch.from_numpy(en))
        raw = wire(idx, vals, 0.0 if bad else (1.0 if weight is None else weight), 0.0 if bad else 1.0, world, S, k)
        image[:, slot].copy_(torch.from_numpy(raw))

    @staticmethod
    def topk_decode(image, nclients, chunk_stride, S, first, first_step, g16, g32, layout, out, out_stride, k):
        assert layout in ("plain", "weighted")
        raw = image.numpy()
        g = _cat(g16, g32)
        n = g.size
        nbk = S // B * k
        for c in range(nclients):
            ch = raw[c * chunk_stride:c * chunk_stride + topk_chunk_bytes(S, k)]
            vals, idx = ch[:4 * nbk].view(F32).reshape(-1, k), ch[4 * nbk:5 * nbk].reshape(-1, k)
            w, vote = ch[-8:].view(F32)
            i = first + c * first_step + np.arange(S)
            if vote == 0:
                y = np.zeros(S, F32)
            else:
                gi = np.where(i < n, g[np.minimum(i, n - 1)], F32(0))
                yy = gi + scatter(idx, vals)
                y = np.where(i < n, w * yy if layout == "weighted" else yy, F32(0)).astype(F32)
                y[i == n] = vote if layout == "plain" else w
                if layout != "plain":
                    y[i == n + 1] = vote
            out[c * out_stride:c * out_stride + S].copy_(torch.from_numpy(y))


class TopkFedOptKernels(TopkHostKernels, FedOptHostKernels):
    """... with the server step."""


# ----------------------------------------------------------------------------- the selection rule, by hand

def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def test_hand_worked_blocks():
    """Blocks whose ranks are known without any sort: a tie between opposite signs at the k-th place (the lower index
    wins), an all-equal block (its k lowest indices), an all-zero block, and a -0.0 among zeros (kept with its sign
    when its index is below k, left in the residual with its sign otherwise)."""
    u = np.full(B, 0.5, F32)
    u[200], u[10], u[100], u[3] = -7.0, 5.0, -2.0, 2.0
    idx, vals, en = select_blocks(u[None], 3)
    assert idx.tolist() == [[3, 10, 200]] and vals.tolist() == [[2.0, 5.0, -7.0]]
    want = u.copy()
    want[[3, 10, 200]] = 0.0
    assert np.array_equal(_bits(en[0]), _bits(want)) and en[0, 100] == -2.0
    idx, vals, _ = select_blocks(u[None], 4)  # one more: the other half of the tie
    assert idx.tolist() == [[3, 10, 100, 200]] and vals.tolist() == [[2.0, 5.0, -2.0, -7.0]]
    idx, vals, _ = select_blocks(u[None], 6)  # then the 0.5s from the left
    assert idx.tolist() == [[0, 1, 3, 10, 100, 200]]
    # all equal in magnitude, the signs alternating
    eq = np.where(np.arange(B) % 2 == 0, F32(1.0), F32(-1.0)).astype(F32)
    idx, vals, en = select_blocks(eq[None], 5)
    assert idx.tolist() == [[0, 1, 2, 3, 4]] and vals.tolist() == [[1.0, -1.0, 1.0, -1.0, 1.0]]
    assert not en[0, :5].any() and np.array_equal(en[0, 5:], eq[5:])
    # all zero
    idx, vals, en = select_blocks(np.zeros((1, B), F32), 8)
    assert idx.tolist() == [list(range(8))] and not _bits(vals).any() and not _bits(en).any()
    # -0.0 among zeros
    z = np.zeros(B, F32)
    z[5] = z[100] = -0.0
    idx, vals, en = select_blocks(z[None], 8)
    assert idx.tolist() == [list(range(8))]
    assert _bits(vals)[0].tolist() == [0, 0, 0, 0, 0, 0x80000000, 0, 0]
    assert _bits(en)[0, 5] == 0 and _bits(en)[0, 100] == 0x80000000 and np.count_nonzero(_bits(en)) == 1
    # inf and NaN have a place in the order: above every finite value, NaN above inf
    w = u.copy()
    w[77], w[78] = np.inf, np.nan
    idx, _, _ = select_blocks(w[None], 3)
    assert idx.tolist() == [[77, 78, 200]]
    # through the whole restatement: a block past n sends the indices 0 .. k - 1 with value 0
    idx, vals, en = host_select(u[:20], np.zeros(20, F32), np.zeros(20, F32), False, 3, 2 * B)
    assert idx.tolist() == [[0, 3, 10], [0, 1, 2]] and not vals[1].any() and en.size == 20


def _sample_update(n, seed):
    g = np.random.default_rng(seed)
    u = (g.standard_normal(n) * np.exp2(g.integers(-8, 3, n))).astype(F32)
    u[B:2 * B] = 0                      # an all-zero block
    u[2 * B:3 * B] = F32(0.25)          # an all-equal block
    u[3 * B + 7] = u[3 * B + 9] = F32(1e6)
    u[3 * B + 8] = F32(-1e6)            # a tie at the top
    return u


@pytest.mark.parametrize("k", [1, 3, 8, 64])
def test_conservation_and_contraction(k):
    """For every coordinate s_i + e'_i == u_i and s_i * e'_i == 0: an update is sent whole or kept whole.  Per block,
    in fp64, ||e'||^2 <= (1 - k / 256) ||u||^2: the k largest squares are at least k / 256 of the sum, the
    delta-compressor property the convergence proof of Stich et al. needs."""
    n = 40 * B + 17
    u = _sample_update(n, 1)
    padded = 41 * B
    idx, vals, en = host_select(u, np.zeros(n, F32), np.zeros(n, F32), False, k, padded)
    s = scatter(idx, vals)
    assert not s[n:].any()
    s = s[:n]
    assert np.array_equal(s + en, u) and not (s * en).any()
    assert np.array_equal(np.sort(idx, axis=1), idx) and (np.diff(idx.astype(int), axis=1) > 0).all()
    up = np.zeros(padded, np.float64)
    up[:n] = u
    ep = np.zeros(padded, np.float64)
    ep[:n] = en
    nu, ne = (up.reshape(-1, B) ** 2).sum(1), (ep.reshape(-1, B) ** 2).sum(1)
    assert (ne <= (1.0 - k / B) * nu * (1.0 + 1e-12)).all()
    assert ne[1] == 0 and idx[1].tolist() == list(range(k))  # the all-zero block
    assert idx[2].tolist() == list(range(k))                  # the all-equal block
    assert idx[3].tolist() == [7] if k == 1 else {7, 8, 9} <= set(idx[3].tolist())  # the tie at the top


def test_nothing_is_ever_lost():
    """g = 0 and x = d_r, integers in [-64, 64] times 2^-12 (exact in fp16 and in every fp32 sum here), k = 8, 40
    rounds: what was sent plus what is still in the residual is everything that was ever to be sent, bit for bit."""
    n = 4868
    rng = np.random.default_rng(7)
    g = np.zeros(n, F32)
    e = np.zeros(n, F32)
    sent, due = np.zeros(n, F32), np.zeros(n, F32)
    padded = -(-n // B) * B
    for _ in range(40):
        d = (rng.integers(-64, 65, n).astype(F32) * F32(2.0 ** -12)).astype(F32)
        assert np.array_equal(d.astype(np.float16).astype(F32), d)
        idx, vals, e = host_select(d, g, e, False, 8, padded)
        sent = sent + scatter(idx, vals)[:n]
        due = due + d
    assert np.array_equal(_bits(sent + e), _bits(due))
    print(f"largest residual after 40 rounds: {np.abs(e).max():.3f}")
    assert 0 < np.abs(e).max() < 1.0


def test_chunk_sizes():
    from federated_multi_modal_amd import _lib, ops
    for S, k, want in ((256, 3, 24), (256, 8, 48), (256, 1, 16), (256, 64, 328), (512, 8, 88), (1536, 3, 100),
                       (1536, 8, 248)):
        assert topk_chunk_bytes(S, k) == want == _lib.call("mf_topk_chunk_bytes", S, k) == ops.topk_chunk_bytes(S, k)
    for S, k in ((0, 8), (-256, 8), (255, 8), (257, 8), (256, 0), (256, 65), (256, -1)):
        assert _lib.call("mf_topk_chunk_bytes", S, k) == -1
    # 40 bytes per block of 256: 25.6 times fewer than fp32, 6.5 times fewer than int8
    assert topk_chunk_bytes(256 * 1000, 8) - 8 == 40 * 1000 and chunk_bytes(256 * 1000) - 8 == 260 * 1000
    with pytest.raises(ValueError, match="multiple of 256"):
        ops.topk_chunk_bytes(100, 8)
    for bad in (0, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="k:"):
            ops.topk_chunk_bytes(256, bad)


# ----------------------------------------------------------------------------- every layout, one set of bits

def expected(n, scen, k=K, error_feedback=True, weights=None, server=None):
    """One process, no exchange: two rounds in numpy / torch fp32.  Returns ([n_valid per round], flat16, flat32,
    [residual per client]).  Nothing here depends on the world size: the padding only adds all-zero blocks."""
    ge = global_engine()
    g16, g32 = ge.flat16.clone(), ge.flat32.clone()
    padded = padded_for(1, 1 if weights is None else 2)
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
            idx, vals, en = host_select(_cat(p16, p32), g, res[c], out, k, padded)
            if error_feedback:
                if out:
                    assert np.array_equal(en.view(np.int32), res[c].view(np.int32))  # untouched
                res[c] = en
            if not out:
                rows.append(torch.from_numpy(host_dense(g, idx, vals)))
                ws.append(torch.tensor(1.0 if weights is None else weights[c], dtype=torch.float32))
        valid.append(len(rows))
        if not rows:
            continue
        acc = div = None
        for y, w in zip(rows, ws):
            term = y * w if weights is not None else y
            acc = term if acc is None else acc + term
            div = w.clone() if div is None else div + w
        if server is not None:
            sx, sm, sv = host_step(server, acc, div, sx, sm, sv, **HP)
            v = sx.half()
        else:
            v = (acc / div).half()
        g16, g32 = v[:N16].clone(), v[N16:].float()
    return valid, g16, g32, res


def run_rounds(ids, scen, k=K, error_feedback=True, weights=None, server=None, kernels="host", device=None, **bkw):
    """The same two rounds through FedAvgBucket / FedAvgExchange for the clients `ids` of this process.  kernels: the
    host restatement, or None for the bucket's default (the device kernels; the GPU tier)."""
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange, ServerOptimizer
    if kernels == "host":
        kernels = TopkFedOptKernels if server is not None else TopkHostKernels
    engines = [global_engine() for _ in ids]
    if device is not None:
        for e in engines:
            e.device, e.flat16, e.flat32 = device, e.flat16.to(device), e.flat32.to(device)
    kw = dict(bkw) if kernels is None else dict(bkw, kernels=kernels)
    sv = None if server is None else ServerOptimizer(server, engines[0], **HP)
    feds = [FedAvgBucket(e, compress="topk", compress_k=k, error_feedback=error_feedback, client=c,
                         weight=None if weights is None else weights[c], server=sv, **kw)
            for e, c in zip(engines, ids)]
    x = FedAvgExchange(feds, **{key: v for key, v in bkw.items() if key in ("mode", "shard_single")})
    assert x.chunk == topk_chunk_bytes(x.S, k) and x.image.shape == (x.world, len(ids), x.chunk)
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


WEIGHTS = (3.0, 1.0, 2.0, 0.5, 1.5, 4.0)
# (name, run_rounds / expected keywords): k = 3 makes a shard's entries no multiple of 4 at three ranks
VARIANTS = [("k3", dict(k=3)), ("k64", dict(k=64)), ("no_feedback", dict(error_feedback=False)),
            ("weighted", dict(weights=WEIGHTS)), ("fedadam", dict(server="fedadam")),
            ("weighted_fedavgm", dict(weights=WEIGHTS, server="fedavgm"))]


def cases(n, which):
    if which == "allreduce":
        return [(name, scen, {"mode": "allreduce"}) for name, scen in scenarios(n).items()]
    return [(name, scen, {}) for name, scen in scenarios(n).items()] + [(name, scenarios(n)["bad"], kw)
                                                                       for name, kw in VARIANTS]


def _worker(rank, world, port, per_rank, which, out):
    _init(rank, world, port)
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    out[rank] = {name: run_rounds(ids, scen, **kw) for name, scen, kw in cases(world * per_rank, which)}
    dist.destroy_process_group()


@pytest.mark.parametrize("world,per_rank", [(2, 1), (3, 1), (2, 2), (3, 2)])
def test_sparsified_exchange_is_bit_exact_at_every_layout(world, per_rank):
    """Two consecutive rounds (the residual carries over): clean, an invalid client, a late failure (the residual
    applied once) and nobody valid; k = 3 and 64, no error feedback, client weights and a server optimizer with an
    invalid client in round 0.  Every world size and clients-per-rank layout ends with the fp16 weights, residuals and
    n_valid of the one restatement, which knows no world size, and so does the same client set in one process."""
    n = world * per_rank
    if world == 3:
        assert (padded_for(3, 1) // 3 // B * 3) % 4 != 0  # k3: the index region is padded
    res = _spawn(_worker, world, per_rank, "ordered")
    for name, scen, kw in cases(n, "ordered"):
        want = expected(n, scen, **kw)
        assert want[0][-1] == (0 if name == "nobody" else n) and want[0][0] == n - (name in ("bad", "late") or bool(kw))
        for r in range(world):
            ids = range(r * per_rank, (r + 1) * per_rank)
            check((res[r][name][0], list(zip(ids, res[r][name][1]))), want, (name, r))
        one = run_rounds(list(range(n)), scen, **kw)
        check((one[0], list(enumerate(one[1]))), want, (name, "one process"))
        if kw.get("error_feedback", True):
            assert any(e.any() for e in want[3])
        if name == "nobody":  # round 1 kept round 0's global weights, and every residual
            first = expected(n, scen[:1])
            assert torch.equal(want[1], first[1]) and torch.equal(want[2], first[2])
            assert all(np.array_equal(a, b) for a, b in zip(want[3], first[3]))


@pytest.mark.parametrize("n", [1, 2])
def test_one_process(n):
    """World 1: one client and two, every scenario and variant."""
    for name, scen, kw in cases(n, "ordered"):
        one = run_rounds(list(range(n)), scen, **kw)
        check((one[0], list(enumerate(one[1]))), expected(n, scen, **kw), name)


def test_allreduce_mode_decodes_locally():
    """"allreduce" decodes every bucket locally and then sums as before (no traffic is saved).  Two ranks, where the
    all_reduce's order cannot differ from the client order (a + b), so the bits are the restatement's."""
    res = _spawn(_worker, 2, 1, "allreduce")
    for name, scen, kw in cases(2, "allreduce"):
        want = expected(2, scen)
        for r in range(2):
            check((res[r][name][0], [(r, res[r][name][1][0])]), want, (name, r))
        one = run_rounds([0, 1], scen, mode="allreduce")
        check((one[0], list(enumerate(one[1]))), want, (name, "one process"))


def test_sparsification_changes_the_result_and_the_residual_holds_the_rest():
    """Not vacuous: top-k does not give the plain exchange's weights, k = 256 / 4 keeps more than k = 8, and after one
    clean round every client's residual is its update minus what it sent."""
    scen = scenarios(2)["clean"][:1]
    a, b = expected(2, scen, k=8), expected(2, scen, k=64)
    assert not torch.equal(a[2], b[2])
    ge = global_engine()
    g = _cat(ge.flat16, ge.flat32)
    for c in range(2):
        p16, p32 = local_result(c, 0, ge.flat16, ge.flat32)
        u = _cat(p16, p32) - g
        assert np.count_nonzero(a[3][c]) > np.count_nonzero(b[3][c]) > 0
        kept = a[3][c] == 0
        assert np.array_equal(a[3][c][~kept], u[~kept]) and np.count_nonzero(u[kept]) <= -(-N // B) * 8


# ----------------------------------------------------------------------------- residual handling

def _three(**kw):
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    engines = [global_engine() for _ in range(3)]
    feds = [FedAvgBucket(e, kernels=TopkHostKernels, compress="topk", client=c, **kw) for c, e in enumerate(engines)]
    return engines, feds, FedAvgExchange(feds)


def _train(engines, rnd, bad=()):
    for c, e in enumerate(engines):
        p16, p32 = local_result(c, rnd, e.flat16, e.flat32, c in bad)
        e.flat16.copy_(p16)
        e.flat32.copy_(p32)


def test_late_failure_repack_gives_the_same_entries_and_commits_once():
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
        assert torch.equal(x.image[:, :2], first[:, :2])      # the same values, indices and tails
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


def test_residual_state_dict_and_no_error_feedback(tmp_path):
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
    fresh = _three()[1][1]
    fresh.load_state_dict(torch.load(tmp_path / "resid.pt", weights_only=True))
    assert torch.equal(fresh.resid, feds[0].resid)
    engines, plain, x = _three(error_feedback=False)
    assert all(f.resid is None and f.resid_next is None for f in plain)
    _train(engines, 0)
    for f in plain:
        f.pack()
    x.start()
    x.finish()
    for f in plain:
        f.unpack()
    assert x.n_valid() == 3 and all(f.resid is None and f.resid_next is None for f in plain)
    assert plain[0].state_dict() == {"residual": None}


def test_all_zero_update_sends_zero_entries_and_gives_the_global_weights():
    engines, feds, x = _three()
    for f in feds:
        f.pack()
    img = x.image.numpy()
    nbk = x.S // B * K
    assert not img[:, :, :4 * nbk].any() and (img[:, :, -8:].view(F32) == 1.0).all()  # values 0; weight 1, vote 1
    assert (img[:, :, 4 * nbk:5 * nbk].reshape(1, 3, -1, K) == np.arange(K)).all()    # every block's first K indices
    g = global_engine()
    gcat = torch.cat([g.flat16.float(), g.flat32])
    x.decode_local()
    for f in feds:  # g + 0
        assert torch.equal(f.buf[:N], gcat) and f.buf[N] == 1.0 and not f.pbuf[N + 1:].any()
    x.start()
    x.finish()
    want = ((gcat + gcat + gcat) / 3.0).half()
    for f, e in zip(feds, engines):
        f.unpack()
        assert torch.equal(e.flat16, want[:N16]) and torch.equal(e.flat32, want[N16:].float())
        assert not f.resid.any()


# ----------------------------------------------------------------------------- construction, config, ABI

def test_construction_errors():
    from federated_multi_modal_amd.federated import COMPRESS, FedAvgBucket, FedAvgExchange, FedDynState
    assert COMPRESS == ("int8", "topk")
    T = TopkHostKernels
    for bad_k in (0, 65, -1, 8.0, "8", True, None):
        with pytest.raises(ValueError, match="compress_k"):
            FedAvgBucket(global_engine(), kernels=T, compress="topk", compress_k=bad_k)
    with pytest.raises(ValueError, match="compress_k"):
        FedAvgBucket(global_engine(), kernels=T, compress_k=0)
    with pytest.raises(ValueError, match="stochastic"):
        FedAvgBucket(global_engine(), kernels=T, compress="topk", compress_rounding="stochastic")
    for robust in ("median", "trimmed_mean"):
        with pytest.raises(ValueError, match="robust"):
            FedAvgBucket(global_engine(), kernels=T, compress="topk", robust=robust)
    with pytest.raises(ValueError, match="dp_clip"):
        FedAvgBucket(global_engine(), kernels=T, compress="topk", dp_clip=1.0)
    with pytest.raises(ValueError, match="dyn"):
        FedAvgBucket(global_engine(), kernels=T, compress="topk", dyn=FedDynState(0.1, global_engine(), 3))
    a = FedAvgBucket(global_engine(), kernels=T, compress="topk")
    assert a.compress_k == 8 and a.pbuf.numel() == padded_for(1, 1)
    with pytest.raises(ValueError, match="dp_clip"):
        FedAvgExchange([a], dp_std=0.5)
    for other in (dict(compress="topk", compress_k=4), dict(compress="topk", error_feedback=False),
                  dict(compress="int8")):
        with pytest.raises(ValueError, match="compression settings"):
            FedAvgExchange([a, FedAvgBucket(global_engine(), kernels=T, **other)])
    FedAvgExchange([a, FedAvgBucket(global_engine(), kernels=T, compress="topk", client=0)])  # no bits: one index serves
    # the other options stay as they were: int8 never looks at compress_k, and host kernels without topk_* still serve
    i8 = FedAvgBucket(global_engine(), kernels=CompressHostKernels, compress="int8", compress_k=3)
    assert i8.run() == 1 and i8.exchange.chunk == chunk_bytes(padded_for(1, 1)) and i8.exchange.topk is None
    plain = FedAvgBucket(global_engine(), kernels=HostKernels)
    assert plain.compress is None and plain.run() == 1 and plain.exchange.image is None
    # a bucket used alone creates its exchange before its first pack
    alone = FedAvgBucket(global_engine(), kernels=T, compress="topk", compress_k=3, weight=2.0)
    assert alone.run() == 1 and alone._x.image.shape == (1, 1, topk_chunk_bytes(padded_for(1, 2), 3))


def test_config_keys_and_trainer_validation(tmp_path, capsys):
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
    from federated_multi_modal_amd.trainers import MaPLeFederated
    cfg = get_cfg_default()
    extend_cfg(cfg)
    assert (cfg.FED.COMPRESS, cfg.FED.COMPRESS_TOPK) == ("none", 8)
    cfg.merge_from_list(["FED.COMPRESS", "topk", "FED.COMPRESS_TOPK", 4])
    assert (cfg.FED.COMPRESS, cfg.FED.COMPRESS_TOPK) == ("topk", 4)
    yaml = tmp_path / "c.yaml"
    yaml.write_text("FED:\n  COMPRESS: topk\n  COMPRESS_TOPK: 16\n  COMPRESS_ERROR_FEEDBACK: false\n")
    cfg2 = get_cfg_default()
    extend_cfg(cfg2)
    cfg2.merge_from_file(str(yaml))
    assert (cfg2.FED.COMPRESS, cfg2.FED.COMPRESS_TOPK, cfg2.FED.COMPRESS_ERROR_FEEDBACK) == ("topk", 16, False)

    def trainer():
        tr = MaPLeFederated.__new__(MaPLeFederated)
        tr.num_clients, tr.rank = 4, 0
        tr.cfg = get_cfg_default()
        tr.cfg.SEED = 3
        return tr

    def check(**fed_keys):
        fed = {"COMPRESS": "none", "COMPRESS_ROUNDING": "nearest", "COMPRESS_ERROR_FEEDBACK": True, "COMPRESS_SEED": -1,
               "COMPRESS_TOPK": 8, "DP_CLIP": 0.0, "ROBUST_AGG": "none"}
        fed.update(fed_keys)
        return trainer()._compress_cfg(fed.get)

    four = {"compress": None, "rounding": "nearest", "error_feedback": True, "seed": 3}
    assert check() == four and check(COMPRESS_TOPK=4) == four
    assert check(COMPRESS="int8", COMPRESS_TOPK=4) == dict(four, compress="int8")
    assert check(COMPRESS="topk") == dict(four, compress="topk", k=8)
    assert check(COMPRESS=" TopK ", COMPRESS_TOPK=64, COMPRESS_ERROR_FEEDBACK=False) == dict(
        four, compress="topk", k=64, error_feedback=False)
    assert check(COMPRESS="int8", ROBUST_AGG="median")["compress"] == "int8"  # int8 combines with it as before
    assert capsys.readouterr().out == ""
    for key, fed_keys in (("FED.COMPRESS_TOPK", dict(COMPRESS="topk", COMPRESS_TOPK=0)),
                          ("FED.COMPRESS_TOPK", dict(COMPRESS="topk", COMPRESS_TOPK=65)),
                          ("FED.COMPRESS_TOPK", dict(COMPRESS="topk", COMPRESS_TOPK=2.5)),
                          ("FED.COMPRESS_TOPK", dict(COMPRESS="topk", COMPRESS_TOPK="8")),
                          ("FED.COMPRESS_TOPK", dict(COMPRESS_TOPK=True)),
                          ("FED.COMPRESS_ROUNDING", dict(COMPRESS="topk", COMPRESS_ROUNDING="stochastic")),
                          ("FED.ROBUST_AGG", dict(COMPRESS="topk", ROBUST_AGG="median")),
                          ("FED.ROBUST_AGG", dict(COMPRESS="topk", ROBUST_AGG="trimmed_mean")),
                          ("FED.COMPRESS", dict(COMPRESS="topk", DP_CLIP=1.0)),
                          ("FED.COMPRESS", dict(COMPRESS="top-k"))):
        with pytest.raises(ValueError, match=key):
            check(**fed_keys)
    # the report: int8's line as it always was, top-k's beside it
    for name, kernels, cp in (("int8", CompressHostKernels, dict(four, compress="int8")),
                              ("topk", TopkHostKernels, dict(four, compress="topk", k=8))):
        tr = trainer()
        tr.compress = cp
        tr.fed = [FedAvgBucket(global_engine(), kernels=kernels, compress=name)]
        tr.exchange = FedAvgExchange(tr.fed)
        tr._compress_report()
        log = capsys.readouterr().out
        plain, S = 4 * (N + 1), padded_for(1, 1)
        wire = chunk_bytes(S) if name == "int8" else topk_chunk_bytes(S, 8)
        how = "nearest, error feedback" if name == "int8" else "k = 8 of 256, error feedback"
        assert log.splitlines()[0] == (
            f"[INFO] FedAvg uplink compression {name} ({how}): {wire} bytes per client and round instead of {plain} "
            f"({plain / wire:.2f}x), the downlink stays fp32; this exchange decodes locally (one process or "
            "\"allreduce\"): simulated, no traffic is saved")
        assert "residuals are not checkpointed" in log.splitlines()[1] and len(log.splitlines()) == 2
    assert plain / wire > 20


def test_abi_argument_checks_run_before_any_launch():
    """The entry points' error returns, on the host: no device is touched."""
    from federated_multi_modal_amd import _lib, ops
    F = 4  # any non-null, 4-byte aligned address: every call below returns before it is read
    S, k = 512, 8
    ch = topk_chunk_bytes(S, k)
    q = dict(x16=F, g16=F, n16=8, x32=F, g32=F, n32=8, e_in=F, e_out=8, flag=F, weight=1.0, k=k, image=F, stride=ch, S=S,
             world=1)
    d = dict(image=F, stride=ch, nclients=2, S=S, first=0, step=0, g16=F, n16=8, g32=F, n32=8, layout=0, out=F,
             ostride=S, k=k)
    for name, base, change, text in (
            ("mf_topk_select", q, dict(image=None), "null image"),
            ("mf_topk_select", q, dict(flag=None), "null image or flag"),
            ("mf_topk_select", q, dict(x16=None), "null weights"),
            ("mf_topk_select", q, dict(g32=None), "global copy"),
            ("mf_topk_select", q, dict(e_out=None), "residual"),
            ("mf_topk_select", q, dict(e_in=None), "residual"),
            ("mf_topk_select", q, dict(e_out=F), "residual"),
            ("mf_topk_select", q, dict(S=500), "multiple of 256"),
            ("mf_topk_select", q, dict(S=0), "multiple of 256"),
            ("mf_topk_select", q, dict(S=-256), "multiple of 256"),
            ("mf_topk_select", q, dict(k=0), "k outside"),
            ("mf_topk_select", q, dict(k=65), "k outside"),
            ("mf_topk_select", q, dict(k=-8), "k outside"),
            ("mf_topk_select", q, dict(n16=-1), "negative"),
            ("mf_topk_select", q, dict(n32=-1), "negative"),
            ("mf_topk_select", q, dict(n32=S), "shorter"),
            ("mf_topk_select", q, dict(world=0), "world"),
            ("mf_topk_select", q, dict(weight=0.0), "weight"),
            ("mf_topk_select", q, dict(weight=float("nan")), "weight"),
            ("mf_topk_select", q, dict(weight=float("inf")), "weight"),
            ("mf_topk_select", q, dict(image=6), "misaligned"),
            ("mf_topk_select", q, dict(world=2, n32=S, stride=ch - 4), "stride"),
            ("mf_topk_decode", d, dict(image=None), "null"),
            ("mf_topk_decode", d, dict(out=None), "null"),
            ("mf_topk_decode", d, dict(g16=None), "global copy"),
            ("mf_topk_decode", d, dict(S=300), "multiple of 256"),
            ("mf_topk_decode", d, dict(k=0), "k outside"),
            ("mf_topk_decode", d, dict(k=65), "k outside"),
            ("mf_topk_decode", d, dict(n32=-1), "negative"),
            ("mf_topk_decode", d, dict(first=-1), "negative"),
            ("mf_topk_decode", d, dict(step=-1), "negative"),
            ("mf_topk_decode", d, dict(nclients=0), "nclients"),
            ("mf_topk_decode", d, dict(layout=2), "layout"),
            ("mf_topk_decode", d, dict(layout=-1), "layout"),
            ("mf_topk_decode", d, dict(stride=ch - 4), "stride"),
            ("mf_topk_decode", d, dict(ostride=S - 1), "stride"),
            ("mf_topk_decode", d, dict(image=5), "misaligned")):
        args = dict(base)
        args.update(change)
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call(name, *args.values(), None)  # the stream last
    p16, p32 = torch.zeros(8, dtype=torch.float16), torch.zeros(8)
    g16, g32, flag = p16.clone(), p32.clone(), torch.zeros(1, dtype=torch.int32)
    e_in, e_out, image = torch.zeros(16), torch.zeros(16), torch.zeros(1, 2, ch, dtype=torch.uint8)
    for kw, text in ((dict(k=0), "k:"), (dict(k=65), "k:"), (dict(k=8.0), "k:"), (dict(k=True), "k:"),
                     (dict(weight=0.0), "weight"), (dict(g16=g16[:4]), "g16"), (dict(S=100), "multiple of 256"),
                     (dict(image=image.float()), "image"), (dict(image=image[:, :, :ch - 4]), "image"),
                     (dict(slot=2), "slot"), (dict(S=256), "image"), (dict(k=4), "image"),
                     (dict(e_out=None), "both"), (dict(e_out=e_in), "overlaps"), (dict(e_in=e_in[:8]), "e_in"),
                     (dict(invalid_flag=None), "invalid_flag"),
                     (dict(p32=torch.zeros(1024), g32=torch.zeros(1024)), "hold fewer")):
        a = dict(p16=p16, p32=p32, g16=g16, g32=g32, e_in=e_in, e_out=e_out, invalid_flag=flag, weight=None, k=k,
                 image=image, slot=0, S=S)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.topk_select(**a)
    flat, out = image.view(-1), torch.zeros(2 * S)
    for kw, text in ((dict(layout="robust"), "layout"), (dict(layout="median"), "layout"), (dict(k=0), "k:"),
                     (dict(S=100), "multiple of 256"), (dict(nclients=0), "nclients"), (dict(first=-1), "first"),
                     (dict(nclients=3), "image"), (dict(out=out[:S]), "out"), (dict(out=out.double()), "out"),
                     (dict(chunk_stride=ch - 4), "chunk_stride"), (dict(out_stride=S - 4), "out_stride"),
                     (dict(g16=g32), "g16")):
        a = dict(image=flat, nclients=2, chunk_stride=ch, S=S, first=0, first_step=0, g16=g16, g32=g32, layout="plain",
                 out=out, out_stride=S, k=k)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.topk_decode(**a)
