"""GPU tier: the DP-FedAvg kernels (mf_dp_update_scale, mf_fedavg_pack_clipped, mf_dp_add_noise) against the host
restatements of tests/test_fedavg_dp_dist.py -- the clipped pack bit for bit, the norm and the normals against fp64
within bounds derived below -- then through FedAvgBucket / FedAvgExchange on the device (one process, and the RCCL
chain in a one-rank group), with a server optimizer, and through the trainer.

Bounds.  Norm: each thread adds at most 32 + 8 squares in fp32 (a chunk is 8192 elements over 256 threads; the ragged
ends add a few), the wave and block sums 6 + 3 more, the second stage runs in fp64: under 41 * 2^-24 = 2.5e-6
relative on the sum of squares, half that on the norm; gate 1e-5.  Normals: r <= sqrt(2 * 24 * ln 2) = 5.77; theta
carries 2^-24 relative from the product's rounding and 2.8e-8 from 6.2831855f against 2 pi, 5.5e-7 absolute at most,
sinf / cosf and logf / sqrtf a few ulps, so |z - z64| <= 5.77 * 5.5e-7 + 5 * 2^-24 * 5.77 + ... about 7.5e-6;
gate 2e-5."""
import math
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

from federated_multi_modal_amd import _lib, ops
from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange, ServerOptimizer, dp_epsilon
from federated_multi_modal_amd.trainers import build_trainer
from test_fedavg_dp_dist import host_clipped, host_normals64
from test_fedavg_robust_dist import QNAN_BITS
from test_fedopt_dist import HP, _f, host_step
from test_fedprox_weighted_gpu import small_cfg

pytestmark = pytest.mark.gpu

SHAPES = [(37, 4099), (0, 5), (4096, 0), (8200, 8)]
NOISE_GATE = 2e-5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pair(n16, n32, seed, scale=1.0):
    """(p16, g16, p32, g32) on the CPU: weights over a few binades and an update of about 1e-2 of them."""
    g = torch.Generator().manual_seed(seed)
    g16 = torch.randn(n16, generator=g).half()
    g32 = torch.randn(n32, generator=g) * torch.exp2(torch.randint(-4, 4, (n32,), generator=g).float())
    p16 = (g16.float() + scale * 1e-2 * torch.randn(n16, generator=g)).half()
    p32 = g32 + scale * 1e-2 * torch.randn(n32, generator=g)
    return p16, g16, p32, g32


def _at(t, off, dev):
    """t on the device, `off` elements past an aligned allocation."""
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device=dev)
    buf[off:].copy_(t)
    return buf[off:]


def _scale(dev, p16, g16, p32, g32, clip):
    ws = torch.zeros(ops.dp_update_ws_floats(p16.numel(), p32.numel()), device=dev)
    out = torch.full((3,), -7.0, device=dev)
    ops.dp_update_scale(p16, g16, p32, g32, clip, ws, out)
    return out


# ----------------------------------------------------------------------------- mf_dp_update_scale

@pytest.mark.parametrize("n16,n32", SHAPES)
def test_update_scale(dev, n16, n32):
    """The four shapes (below a chunk, an empty buffer either side, the chunk boundary); pointers aligned, both one
    element off (vector loads after a ragged head) and the weights alone one element off (element loads throughout)."""
    cpu = _pair(n16, n32, 7 * n16 + n32)
    d = torch.cat([cpu[0].float() - cpu[1].float(), cpu[2] - cpu[3]])
    want = float(torch.sqrt((d.double() ** 2).sum()))
    worst = 0.0
    for offs in ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (3, 3, 2, 2)):
        p16, g16, p32, g32 = (_at(t, o, dev) for t, o in zip(cpu, offs))
        outs = []
        for clip in (want * 4.0, want * 0.25):
            out = _scale(dev, p16, g16, p32, g32, clip)
            again = _scale(dev, p16, g16, p32, g32, clip)
            assert torch.equal(_bits(out), _bits(again)), (offs, clip)  # run to run
            outs.append(out.cpu())
        (norm, s_in, f_in), (norm2, s_out, f_out) = outs[0].tolist(), outs[1].tolist()
        assert norm == norm2
        rel = abs(norm - want) / want
        worst = max(worst, rel)
        print(f"dp_update_scale ({n16}, {n32}) offsets {offs}: norm {norm!r}, fp64 {want!r}, rel {rel:.3e}")
        assert rel <= 1e-5, (offs, norm, want)
        assert s_in == 1.0 and f_in == 0.0
        clip32 = torch.tensor(want * 0.25, dtype=torch.float32)
        assert _bits(outs[1][1]) == _bits(clip32 / outs[1][0]) and f_out == 1.0 and s_out < 1.0
        # a bound equal to the norm is not exceeded
        at = _scale(dev, p16, g16, p32, g32, norm).tolist()
        assert at == [norm, 1.0, 0.0]
    print(f"dp_update_scale ({n16}, {n32}): max relative norm error {worst:.3e}")
    # a NaN norm clips nothing: the validity flag deals with that client
    p16, g16, p32, g32 = (t.to(dev) for t in cpu)
    (p32 if n32 else p16)[0] = float("nan")
    out = _scale(dev, p16, g16, p32, g32, 1.0).tolist()
    assert math.isnan(out[0]) and out[1:] == [1.0, 0.0]
    # no update at all
    assert _scale(dev, g16, g16.clone(), g32, g32.clone(), 1.0).tolist() == [0.0, 1.0, 0.0]


# ----------------------------------------------------------------------------- mf_fedavg_pack_clipped

LAYOUTS = (("plain", None), ("weighted", 2.5), ("robust", None))


def _host_bucket(cpu, s, layout, weight):
    p16, g16, p32, g32 = cpu
    y = host_clipped(p16, p32, g16, g32, s)
    if layout == "plain":
        return torch.cat([y, torch.ones(1)])
    w = torch.tensor(weight if layout == "weighted" else 1.0, dtype=torch.float32)
    return torch.cat([y * w, w.reshape(1), torch.ones(1)])


@pytest.mark.parametrize("n16,n32", SHAPES)
def test_pack_clipped(dev, n16, n32):
    cpu = _pair(n16, n32, 11 * n16 + n32)
    if n32:
        cpu[2][0] = -0.0
    p16, g16, p32, g32 = (t.to(dev) for t in cpu)
    n = n16 + n32
    g = torch.cat([cpu[1].float(), cpu[3]])
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    norm = _scale(dev, p16, g16, p32, g32, 1e30)[0].item()
    for layout, weight in LAYOUTS:
        tail = 1 if layout == "plain" else 2
        # the three-operation path: the device's own scale, read back
        clip = 0.3 * norm
        out = _scale(dev, p16, g16, p32, g32, clip)
        s = out[1:2].cpu()
        assert float(s) < 1.0
        bucket = torch.full((n + tail,), 5.0, device=dev)
        flag.zero_()
        ops.fedavg_pack_clipped(p16, p32, g16, g32, flag, out[1:2], weight, layout, bucket)
        want = _host_bucket(cpu, s[0], layout, weight)
        assert torch.equal(_bits(bucket), _bits(want)), layout
        y = host_clipped(*[cpu[i] for i in (0, 2, 1, 3)], s[0])
        bound = clip * (1 + 1e-5) + math.sqrt(n) * 2.0 ** -24 * float(y.abs().max())
        assert float((y.double() - g.double()).norm()) <= bound, layout
        # inside the bound: the select, and the bits of the existing pack kernels
        out = _scale(dev, p16, g16, p32, g32, 4.0 * norm)
        assert out[1].item() == 1.0
        ops.fedavg_pack_clipped(p16, p32, g16, g32, flag, out[1:2], weight, layout, bucket)
        plain = torch.full((n + tail,), 6.0, device=dev)
        if layout == "plain":
            ops.fedavg_pack(p16, p32, flag, plain)
        elif layout == "weighted":
            ops.fedavg_pack_weighted(p16, p32, flag, weight, plain)
        else:
            ops.fedavg_pack_robust(p16, p32, flag, plain)
        assert torch.equal(_bits(bucket), _bits(plain)), layout
        assert torch.equal(_bits(bucket), _bits(_host_bucket(cpu, torch.ones(()), layout, weight))), layout
        # an invalid client: zeros, or all quiet NaNs in the robust layout, whatever the scale
        flag.fill_(1)
        for sc in (out[1:2], s.to(dev)):
            bucket.fill_(5.0)
            ops.fedavg_pack_clipped(p16, p32, g16, g32, flag, sc, weight, layout, bucket)
            assert (_bits(bucket) == (QNAN_BITS if layout == "robust" else 0)).all(), layout
    with pytest.raises(ValueError, match="bucket"):
        ops.fedavg_pack_clipped(p16, p32, g16, g32, flag, out[1:2], None, "plain", bucket)  # a robust-sized bucket


# ----------------------------------------------------------------------------- mf_dp_add_noise

SENTINEL = 12345.0


def _noised(dev, n, offset, seed, rnd, std, misalign=0, shards=None, fill=0.0):
    """A buffer of n floats `misalign` floats past an aligned allocation, sentinels either side, noised in one call
    or in the given (start, length) shards; returns the n values after checking the sentinels."""
    whole = torch.full((n + misalign + 16,), SENTINEL, device=dev)
    buf = whole[8 + misalign:8 + misalign + n]
    buf.fill_(fill)
    for start, length in shards or [(0, n)]:
        ops.dp_add_noise(buf[start:start + length], offset + start, seed, rnd, std)
    out = whole.cpu()
    assert (out[:8 + misalign] == SENTINEL).all() and (out[8 + misalign + n:] == SENTINEL).all()
    return out[8 + misalign:8 + misalign + n]


@pytest.mark.parametrize("base", [0, 3, 2 ** 34 + 1])
def test_noise_is_layout_independent_and_stays_in_range(dev, base):
    """One call over n = 1031 equals the calls over its shards at 0, 257, 514 and 771 (starts that are no multiples
    of 4: partial first and last counters, 16-byte and element accesses mixed), on an aligned buffer and on one a
    float off; no element outside [0, n) is written; a base at or above 2^34 uses the counter's high word."""
    n, shards = 1031, [(0, 257), (257, 257), (514, 257), (771, 260)]
    one = _noised(dev, n, base, 99, 5, 0.75, fill=1.0)
    for misalign in (0, 1, 2):
        assert torch.equal(_bits(_noised(dev, n, base, 99, 5, 0.75, misalign, fill=1.0)), _bits(one)), misalign
        assert torch.equal(_bits(_noised(dev, n, base, 99, 5, 0.75, misalign, shards, fill=1.0)), _bits(one)), misalign
    for tiny in (1, 2, 3, 5):  # calls shorter than a counter
        got = _noised(dev, tiny, base + 2, 99, 5, 0.75, fill=1.0)
        assert torch.equal(_bits(got), _bits(one[2:2 + tiny])), tiny
    z64 = host_normals64(np.uint64(base) + np.arange(n, dtype=np.uint64), 99, 5)
    assert np.abs(one.double().numpy() - (1.0 + 0.75 * z64)).max() <= 0.75 * NOISE_GATE + 2.0 ** -22
    assert not torch.equal(one, _noised(dev, n, base, 100, 5, 0.75, fill=1.0))  # another seed
    assert not torch.equal(one, _noised(dev, n, base, 99 + 2 ** 32, 5, 0.75, fill=1.0))  # the seed's high word
    assert not torch.equal(one, _noised(dev, n, base, 99, 6, 0.75, fill=1.0))   # another round
    # std = 0 leaves the bits, a -0 included
    buf = torch.tensor([-0.0, 1.5, -2.0, 0.0], device=dev)
    ops.dp_add_noise(buf, base, 99, 5, 0.0)
    assert _bits(buf).tolist() == _bits(torch.tensor([-0.0, 1.5, -2.0, 0.0])).tolist()


@pytest.fixture(scope="module")
def normals(dev):
    """2^20 normals of seed 1234 at rounds 1 and 2 from the device (zeros + std 1), and the fp64 reference of round 1."""
    n = 1 << 20
    z1 = _noised(dev, n, 0, 1234, 1, 1.0).double().numpy()
    z2 = _noised(dev, n, 0, 1234, 2, 1.0).double().numpy()
    return z1, z2, host_normals64(np.arange(n, dtype=np.uint64), 1234, 1)


def test_noise_accuracy(normals):
    """Against the fp64 Box-Muller of the exact uniforms; a wrong Philox word moves a normal by far more than the
    gate, so this pins the generator too."""
    z1, _, ref = normals
    err = np.abs(z1 - ref).max()
    print(f"dp_add_noise: max |z - z64| over 2^20 normals = {err:.3e}, max |z| = {np.abs(z1).max():.4f}")
    assert err <= NOISE_GATE


def test_noise_statistics(normals):
    """Each within 5 sigma of a standard normal's value over 2^20 samples (the fp64 reference alone gives -3.6e-4,
    0.99909, 2.9987, 1.9e-3, -1.1e-3 for this seed; the generator is seeded, so nothing here can flake)."""
    z1, z2, _ = normals
    mean, var = z1.mean(), z1.var()
    kurt = ((z1 - mean) ** 4).mean() / var ** 2
    lag1 = np.corrcoef(z1[:-1], z1[1:])[0, 1]
    cross = np.corrcoef(z1, z2)[0, 1]
    print(f"dp_add_noise statistics: mean {mean:.3e}, var {var:.5f}, kurtosis {kurt:.4f}, lag-1 {lag1:.3e}, "
          f"round 1 x round 2 {cross:.3e}")
    assert abs(mean) <= 4.9e-3
    assert abs(var - 1.0) <= 6.9e-3
    assert abs(kurt - 3.0) <= 2.4e-2
    assert abs(lag1) <= 4.9e-3
    assert abs(cross) <= 4.9e-3


def test_argument_errors(dev):
    """Every error returns before any launch: the outputs keep their bits."""
    P, S = ops._p, ops._s
    p16, g16 = torch.zeros(8, dtype=torch.float16, device=dev), torch.zeros(8, dtype=torch.float16, device=dev)
    p32, g32 = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    ws, out, bucket = torch.zeros(2, device=dev), torch.full((3,), 9.0, device=dev), torch.full((18,), 9.0, device=dev)
    for name, args, text in (
            ("mf_dp_update_scale", (P(p16), P(g16), -1, P(p32), P(g32), 8, 1.0, P(ws), P(out), S()), "negative"),
            ("mf_dp_update_scale", (P(p16), P(g16), 8, P(p32), P(g32), 8, 0.0, P(ws), P(out), S()), "clip"),
            ("mf_dp_update_scale", (P(p16), P(g16), 8, P(p32), P(g32), 8, -1.0, P(ws), P(out), S()), "clip"),
            ("mf_dp_update_scale", (P(p16), P(g16), 8, P(p32), None, 8, 1.0, P(ws), P(out), S()), "global copy"),
            ("mf_fedavg_pack_clipped", (P(p16), 8, P(p32), 8, P(g16), P(g32), None, P(out), 1.0, 3, P(bucket), S()),
             "layout"),
            ("mf_fedavg_pack_clipped", (P(p16), 8, P(p32), 8, P(g16), P(g32), None, P(out), -1.0, 1, P(bucket), S()),
             "weight"),
            ("mf_fedavg_pack_clipped", (P(p16), 8, P(p32), 8, P(g16), P(g32), None, None, 1.0, 0, P(bucket), S()),
             "scale"),
            ("mf_dp_add_noise", (P(bucket), -1, 0, 1, 0, 1.0, S()), "negative"),
            ("mf_dp_add_noise", (P(bucket), 18, -1, 1, 0, 1.0, S()), "negative"),
            ("mf_dp_add_noise", (P(bucket), 18, 2 ** 63 - 2, 1, 0, 1.0, S()), "overflow"),
            ("mf_dp_add_noise", (P(bucket), 18, 0, 1, 0, float("nan"), S()), "std")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call(name, *args)
    with pytest.raises(ValueError, match="overlaps"):
        ops.dp_update_scale(p16, g16, p32, g32, 1.0, ws, p32[:3])
    with pytest.raises(ValueError, match="std"):
        ops.dp_add_noise(bucket, 0, 1, 0, -1.0)
    torch.cuda.synchronize()
    assert (out == 9.0).all() and (bucket == 9.0).all() and (p32 == 1.0).all()


# ----------------------------------------------------------------------------- FedAvgBucket on the device

N16, N32 = 1003, 7777
N = N16 + N32
CLIP, Z, SEED = 0.25, 1.3, 2 ** 40 + 17
STD = float(np.float32(Z) * np.float32(CLIP))


class _Eng:
    """The global weights (seed 0), or a client's local result: an update of L2 norm about 0.1, 100 x that for `far`."""

    def __init__(self, dev, client=None, far=False):
        g = torch.Generator().manual_seed(0)
        self.device = dev
        self.n16, self.n32 = N16, N32
        f16 = torch.randn(N16, generator=g) * 3
        f32 = torch.randn(N32, generator=g) * 1e-1
        if client is not None:
            g = torch.Generator().manual_seed(10 + client)
            k = 100.0 if far else 1.0
            f16 = f16.half().float() + k * 2e-3 * torch.randn(N16, generator=g)
            f32 = f32 + k * 1e-3 * torch.randn(N32, generator=g)
        self.flat16, self.flat32 = f16.half().to(dev), f32.to(dev)
        self.loaded = 0

    def after_weights_loaded(self):
        self.loaded += 1


def _three_clients(dev, shard_single, server_for=None, invalid=()):
    engines, feds, server = [], [], None
    for c in range(3):
        e = _Eng(dev)
        if server_for is not None and server is None:
            server = ServerOptimizer(server_for, e, **HP)
        feds.append(FedAvgBucket(e, dp_clip=CLIP, shard_single=shard_single, server=server))
        loc = _Eng(dev, c, far=c == 2)  # client 2 is far off, and finite
        e.flat16.copy_(loc.flat16)
        e.flat32.copy_(loc.flat32)
        if c in invalid:
            e.flat32[7] = float("nan")
        engines.append(e)
    return engines, feds, server


def _round(dev, shard_single, server_for=None, invalid=(), rnd=0):
    """One noised round of three clients; returns (exchange, the noised summed bucket, the fp64 restatement of its
    first N floats from the device's own scales, engines, server)."""
    engines, feds, server = _three_clients(dev, shard_single, server_for, invalid)
    glob = _Eng(dev)
    x = FedAvgExchange(feds, shard_single=shard_single, dp_std=STD, dp_seed=SEED)
    x.load_state_dict({"round": rnd, "seed": SEED})
    locals_ = [(e.flat16.cpu(), e.flat32.cpu()) for e in engines]
    for f in feds:
        f.pack()
    x.start()
    x.finish()
    total = feds[0].buf.clone()
    stats = [f.clip_stats() for f in feds]
    acc = None
    for c, ((p16, p32), (norm, s)) in enumerate(zip(locals_, stats)):
        if c in invalid:
            assert math.isnan(norm) and s == 1.0
            row = torch.zeros(N)
        else:
            assert (s < 1.0) == (c == 2) and (norm > CLIP) == (c == 2), (c, norm, s)
            row = host_clipped(p16, p32, glob.flat16.cpu(), glob.flat32.cpu(), torch.tensor(s))
        acc = row if acc is None else acc + row
    want = acc.double().numpy() + STD * host_normals64(np.arange(N, dtype=np.uint64), SEED, rnd)
    for f in feds:
        f.unpack()
    torch.cuda.synchronize()
    assert x.round == rnd + 1
    return x, total.cpu(), (acc, want), engines, server


def _check_noised(total, acc, want, n_valid):
    tol = STD * NOISE_GATE + 2.0 ** -23 * (float(acc.abs().max()) + 6.0 * STD)
    assert np.abs(total[:N].double().numpy() - want).max() <= tol
    assert total[N].item() == n_valid  # the vote: never noised
    assert not torch.equal(total[:N], acc)


@pytest.fixture
def rccl_group(dev):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    yield
    dist.destroy_process_group()


def test_three_clients_in_one_process_and_over_the_rccl_chain(dev, rccl_group):
    """One process (local sum, then the noise over the whole bucket) and all_to_all -> reduce -> noise on the shard ->
    all_gather on the side stream in a one-rank group: both equal the restatement within the noise gate, and each
    other bit for bit; the padding after the vote stays zero."""
    xa, ta, (acc, want), ea, _ = _round(dev, False)
    assert not xa.distributed
    _check_noised(ta, acc, want, 3)
    xb, tb, (acc_b, want_b), eb, _ = _round(dev, True)
    assert xb.sharded and xb.side is not None
    _check_noised(tb, acc_b, want_b, 3)
    assert torch.equal(_bits(ta), _bits(tb))
    val = (ta[:N] / 3.0).half()
    for e in ea + eb:
        assert e.loaded == 1
        assert torch.equal(e.flat16.cpu(), val[:N16]) and torch.equal(e.flat32.cpu(), val[N16:].float())
    # an invalid client, the next round's stream
    _, t1, (acc1, want1), _, _ = _round(dev, True, invalid=(1,), rnd=1)
    _check_noised(t1, acc1, want1, 2)
    _, t1p, _, _, _ = _round(dev, False, invalid=(1,), rnd=1)
    assert torch.equal(_bits(t1), _bits(t1p))
    # nobody valid: the sum is noise alone, the vote 0, and the global copy comes back
    _, t0, _, engines, _ = _round(dev, True, invalid=(0, 1, 2), rnd=2)
    assert t0[N].item() == 0.0 and t0[:N].any()
    glob = _Eng(dev)
    for e in engines:
        assert torch.equal(e.flat16, glob.flat16) and torch.equal(e.flat32, glob.flat32)


def test_server_optimizer_consumes_the_noised_clipped_mean(dev, rccl_group):
    glob = _Eng(dev)
    x0 = torch.cat([glob.flat16.float(), glob.flat32]).cpu()
    _, total, (acc, want), engines, server = _round(dev, True, server_for="fedadam")
    _check_noised(total, acc, want, 3)
    tau2 = float(_f(HP["tau"]) * _f(HP["tau"]))
    xs, m, v = host_step("fedadam", total[:N], total[N], x0, torch.zeros_like(x0), torch.full_like(x0, tau2), **HP)
    assert torch.equal(server.x.cpu(), xs) and torch.equal(server.m.cpu(), m) and torch.equal(server.v.cpu(), v)
    val = xs.half()
    for e in engines:
        assert torch.equal(e.flat16.cpu(), val[:N16]) and torch.equal(e.flat32.cpu(), val[N16:].float())
    assert not torch.equal(xs, x0)


# ----------------------------------------------------------------------------- through the trainer

def _local_results(tr, seed):
    """Stand-ins for local training: every client's weights moved off the global copy by a seeded perturbation."""
    for c in tr.clients:
        g = torch.Generator().manual_seed(1000 * seed + c.client_id)
        e = c.engine
        e.flat16.add_((2.0 ** -6 * torch.randn(e.n16, generator=g)).half().to(e.flat16.device))
        e.flat32.add_((2.0 ** -6 * torch.randn(e.n32, generator=g)).to(e.flat32.device))


def _same_weights(a, b):
    return all(torch.equal(x.engine.flat16, y.engine.flat16) and torch.equal(x.engine.flat32, y.engine.flat32)
               for x, y in zip(a.clients, b.clients))


def test_a_bound_nobody_reaches_is_the_default_run(dev, tmp_path):
    on = build_trainer(small_cfg(tmp_path / "on", clients=2, extra=["FED.DP_CLIP", 1e30, "FED.DP_NOISE_MULTIPLIER", 0]))
    plain = build_trainer(small_cfg(tmp_path / "plain", clients=2))  # no mention of the new keys
    assert all(f.dp_clip == 1e30 for f in on.fed) and all(f.dp_clip is None for f in plain.fed)
    assert on.exchange.dp_std == 0.0 and plain.exchange.dp_std == 0.0
    for rnd in (1, 2):
        _local_results(on, rnd)
        _local_results(plain, rnd)
        assert _same_weights(on, plain)
        assert on._fedavg([]) == 2 and plain._fedavg([]) == 2
        assert _same_weights(on, plain)
        norm, scale = on.fed[0].clip_stats()
        assert scale == 1.0 and norm > 1.0


DP = ["FED.DP_CLIP", 0.5, "FED.DP_NOISE_MULTIPLIER", 1.2, "FED.DP_DELTA", 1e-6]


def test_dp_rounds_through_the_trainer_log(dev, tmp_path, capsys):
    """Two real rounds under DP: the log carries every local client's update norm and whether it was clipped, and a
    cumulative epsilon that grows; the checkpoint carries the noise stream's position."""
    # a learning rate that moves the weights (the config's warm-up rate of 1e-4 moves hardly any fp16 weight), and a
    # bound below any update it can produce
    bound = 1e-5
    tr = build_trainer(small_cfg(tmp_path, clients=2, rounds=2, extra=[
        "FED.DP_CLIP", bound, "FED.DP_NOISE_MULTIPLIER", 1.2, "FED.DP_DELTA", 1e-6, "FED.DP_SEED", 5,
        "OPTIM.WARMUP_CONS_LR", 0.01]))
    assert "[INFO] DP-FedAvg: client updates clipped to L2 norm 1e-05" in capsys.readouterr().out
    assert tr.exchange.dp_seed == 5 and tr.exchange.dp_std == float(np.float32(1.2) * np.float32(bound))
    tr.train()
    out = capsys.readouterr().out
    eps = [float(m) for m in re.findall(r"DP epsilon = ([0-9.eE+-]+) at delta = 1e-06", out)]
    assert eps == [float(f"{dp_epsilon(1.2, r, 1e-6):.6g}") for r in (1, 2)] and eps[1] > eps[0]
    norms = re.findall(r"\[Round (\d)\] DP update norms \(bound 1e-05\): client 0: ([0-9.eE+-]+) \((\w+)[^)]*\), "
                       r"client 1: ([0-9.eE+-]+) \((\w+)", out)
    assert [r[0] for r in norms] == ["1", "2"], out
    for _, n0, how0, n1, how1 in norms:
        assert how0 == ("clipped" if float(n0) > bound else "kept")
        assert how1 == ("clipped" if float(n1) > bound else "kept")
    assert any(how == "clipped" for r in norms for how in (r[2], r[4]))
    assert tr.exchange.round == 2 and tr.dp_rounds == 2
    ckpt = torch.load(tmp_path / "MultiModalPromptLearner_Aggregator" / f"model.pth.tar-{tr.cfg.OPTIM.MAX_EPOCH}",
                      map_location="cpu", weights_only=True)
    assert ckpt["dp"] == {"round": 2, "seed": 5, "aggregated": 2}


def test_seed_and_checkpoint_through_the_trainer(dev, tmp_path):
    """Another DP_SEED gives other weights, the same one the same bits; a checkpoint saved after round 1 and resumed
    gives round 2 bit-identical to the uninterrupted run, where the same weights under a restarted stream (round 0
    again) do not."""
    a = build_trainer(small_cfg(tmp_path / "a", clients=2, extra=DP + ["FED.DP_SEED", 5]))
    b = build_trainer(small_cfg(tmp_path / "b", clients=2, extra=DP + ["FED.DP_SEED", 6]))
    assert (a.exchange.dp_seed, b.exchange.dp_seed) == (5, 6) and _same_weights(a, b)
    epoch = a.cfg.OPTIM.MAX_EPOCH
    a.save_model()  # the initial weights, the stream at round 0
    for tr in (a, b):
        _local_results(tr, 1)
        assert tr._fedavg([]) == 2 and tr.exchange.round == 1
        assert all(f.clip_stats()[1] < 1.0 for f in tr.fed)
    assert not _same_weights(a, b)
    # every local client holds the one global model
    assert torch.equal(a.clients[0].engine.flat16, a.clients[1].engine.flat16)
    # b again from the initial checkpoint, which carries a's seed: a's bits
    b.load_model(str(tmp_path / "a"), epoch=epoch)
    assert b.exchange.state_dict() == {"round": 0, "seed": 5} and b.dp_rounds == 0
    _local_results(b, 1)
    assert b._fedavg([]) == 2 and _same_weights(a, b)
    # round 2: a uninterrupted, b resumed from the checkpoint a wrote after round 1
    a.dp_rounds = 1  # what the round loop counts
    a.save_model()
    _local_results(a, 2)
    assert a._fedavg([]) == 2 and a.exchange.round == 2
    b.load_model(str(tmp_path / "a"), epoch=epoch)
    assert b.exchange.state_dict() == {"round": 1, "seed": 5} and b.dp_rounds == 1
    _local_results(b, 2)
    assert b._fedavg([]) == 2 and b.exchange.round == 2 and _same_weights(a, b)
    # the same weights and inputs under a stream restarted at round 0: other noise
    b.load_model(str(tmp_path / "a"), epoch=epoch)
    b.exchange.load_state_dict({"round": 0, "seed": 5})
    _local_results(b, 2)
    assert b._fedavg([]) == 2 and not _same_weights(a, b)
    with pytest.raises(ValueError, match="FED.DP_CLIP"):
        build_trainer(small_cfg(tmp_path / "bad", clients=2, extra=["FED.DP_NOISE_MULTIPLIER", 1.0]))
    with pytest.raises(ValueError, match="FED.ROBUST_AGG"):
        build_trainer(small_cfg(tmp_path / "bad2", clients=3, extra=DP + ["FED.ROBUST_AGG", "median"]))
