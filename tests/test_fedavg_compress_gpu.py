"""GPU tier: the uplink compression kernels (mf_compress_quantize, mf_compress_decode) against the numpy fp32
restatement of tests/test_fedavg_compress_dist.py, bit for bit -- codes, scales, tail and residual -- then through
FedAvgBucket / FedAvgExchange on the device (one process, and the RCCL chain in a one-rank group), with a server
optimizer, and through the trainer."""
import numpy as np
import pytest
import torch

from federated_multi_modal_amd import ops
from federated_multi_modal_amd.trainers import build_trainer
from test_fedavg_compress_dist import (B, F32, SEED, CompressHostKernels, _cat, chunk_bytes, host_dequant, host_quantize,
                                       run_rounds)
from test_fedavg_dp_gpu import _local_results, _same_weights, rccl_group  # noqa: F401  (rccl_group: a fixture)
from test_fedprox_weighted_gpu import small_cfg

pytestmark = pytest.mark.gpu

SHAPES = [(0, 5), (256, 0), (1000, 777), (4099, 769)]
SENTINEL = 0xAB


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _at(t, off, dev):
    """t on the device, `off` elements past an aligned allocation."""
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device=dev)
    buf[off:].copy_(t)
    return buf[off:]


def _inputs(n16, n32):
    """(x16, g16, x32, g32, e) on the CPU.  Block 0 has no update and no residual (an all-zero block), block 1 one
    large value among small ones (t = -127 there); at (1000, 777) block 3 straddles the fp16 / fp32 boundary, and no
    shape ends on a block boundary once the tail is counted."""
    n = n16 + n32
    gen = torch.Generator().manual_seed(31 * n16 + n32)
    g16 = torch.randn(n16, generator=gen).half()
    g32 = torch.randn(n32, generator=gen) * torch.exp2(torch.randint(-4, 4, (n32,), generator=gen).float())
    upd = 1e-2 * torch.randn(n, generator=gen) * torch.exp2(torch.randint(-3, 3, (n,), generator=gen).float())
    e = 1e-3 * torch.randn(n, generator=gen)
    if n >= 2 * B:
        upd[:B] = 0.0
        e[:B] = 0.0
        upd[B:2 * B] *= 1e-3
        e[B:2 * B] *= 1e-3
        upd[B + 9] = -7.0
    x16 = (g16.float() + upd[:n16]).half()
    x32 = g32 + upd[n16:]
    return x16, g16, x32, g32, e.contiguous()


def _wire(codes, scales, weight, vote, world, S):
    """The bytes of the `world` chunks, [world][chunk]."""
    tail = np.array([weight, vote], dtype=F32)
    return np.stack([np.concatenate([codes[r * S:(r + 1) * S].view(np.uint8),
                                     scales[r * S // B:(r + 1) * S // B].view(np.uint8), tail.view(np.uint8)])
                     for r in range(world)])


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
@pytest.mark.parametrize("n16,n32", SHAPES)
def test_quantize_matches_the_host_restatement(dev, n16, n32, rounding):
    """Codes, scales, tail and e' bit for bit: the buffers 16-byte aligned, all one element off (element accesses
    throughout) and mixed; S for one destination rank and for three; with and without a residual; a valid client, one
    with the validity flag set (what a `failed` client packs as: codes, scales and tail zero, e' = e); the other
    slot of the image and everything around e' untouched."""
    cpu = _inputs(n16, n32)
    x16, g16, x32, g32, e = cpu
    n = n16 + n32
    x, g = _cat(x16, x32), _cat(g16, g32)
    for world in (1, 3):
        padded = -(-(n + 1) // (world * B)) * world * B
        S = padded // world
        chunk = chunk_bytes(S)
        assert ops.compress_chunk_bytes(S) == chunk
        for offs in ((0,) * 6, (1,) * 6, (1, 0, 0, 1, 1, 0)):
            for feedback, bad, weight in ((True, False, None), (False, False, 2.5), (True, True, 2.5)):
                d16, dg16, d32, dg32, de = (_at(t, o, dev) for t, o in zip(cpu, offs))
                whole = torch.full((n + offs[5] + 8,), 77.0, device=dev)
                e_out = whole[offs[5]:offs[5] + n]
                flag = torch.full((1,), int(bad), dtype=torch.int32, device=dev)
                image = torch.full((world, 2, chunk), SENTINEL, dtype=torch.uint8, device=dev)
                ops.compress_quantize(d16, d32, dg16, dg32, de if feedback else None, e_out if feedback else None, flag,
                                      weight, rounding, SEED, 5, 3, image, 1, S)
                codes, scales, en = host_quantize(x, g, e.numpy() if feedback else None, bad, rounding, SEED, 5, 3, padded)
                want = _wire(codes, scales, 0.0 if bad else (weight or 1.0), 0.0 if bad else 1.0, world, S)
                got = image.cpu().numpy()
                where = (world, offs, feedback, bad)
                assert np.array_equal(got[:, 1, :S], want[:, :S]), ("codes",) + where
                assert np.array_equal(got[:, 1, S:S + S // 64], want[:, S:S + S // 64]), ("scales",) + where
                assert np.array_equal(got[:, 1, S + S // 64:], want[:, S + S // 64:]), ("tail",) + where
                assert (got[:, 0] == SENTINEL).all(), where
                out = whole.cpu()
                if feedback:
                    assert np.array_equal(out[offs[5]:offs[5] + n].numpy().view(np.int32), en.view(np.int32)), where
                    assert (out[:offs[5]] == 77.0).all() and (out[offs[5] + n:] == 77.0).all(), where
                    if bad:
                        assert np.array_equal(en, e.numpy())
                else:
                    assert (out == 77.0).all(), where
                assert torch.equal(de.cpu(), e)  # the residual read is never written
                if not bad and n >= 2 * B:
                    assert not codes[:B].any() and scales[0] == 0 and codes[B + 9] == -127
                    assert np.abs(codes[B:2 * B]).sum() <= 127 + B
                if not bad:
                    assert codes[:n].any() and not codes[n:].any()
    # another round, client or seed: other stochastic codes; nearest rounding reads none of them
    if n >= 2 * B:
        base = host_quantize(x, g, None, False, rounding, SEED, 5, 3, padded)[0]
        for args in ((SEED, 6, 3), (SEED, 5, 4), (SEED + 2 ** 32, 5, 3)):
            other = host_quantize(x, g, None, False, rounding, *args, padded)[0]
            assert np.array_equal(base, other) == (rounding == "nearest")


LAYOUTS = (("plain", None), ("weighted", 2.5), ("robust", None))


@pytest.mark.parametrize("layout,weight", LAYOUTS)
def test_decode_matches_the_host_restatement(dev, layout, weight):
    """A valid and an invalid client's chunks for four destination ranks of 512 coordinates, n = 1777: every shard of
    the received image (the tail elements n and n + 1 outside, inside), shards placed so that n or n + 1 is the first
    or the last element or just outside, a 16-byte aligned out and one a float off, and a whole bucket in one call."""
    n16, n32, S, world = 1000, 777, 512, 4
    n = n16 + n32
    x16, g16, x32, g32, e = _inputs(n16, n32)
    chunk = chunk_bytes(S)
    image = torch.zeros(world, 2, chunk, dtype=torch.uint8)
    for slot, bad in ((0, False), (1, True)):
        CompressHostKernels.compress_quantize(x16, x32, g16, g32, None, None, torch.tensor([int(bad)], dtype=torch.int32),
                                              weight, "stochastic", SEED, 2, slot, image, slot, S)
    dimg, dg16, dg32 = image.to(dev), g16.to(dev), g32.to(dev)
    firsts = [r * S for r in range(world)] + [n - S + 1, n - S + 2, n - S, n - 1, n, n + 1, n + 2, 3]
    for first in firsts:
        rank = min(first // S, world - 1)  # any chunk serves: the position decides what is written
        src, dsrc = image[rank].reshape(-1), dimg[rank].reshape(-1)
        want = torch.full((2 * S,), 9.0)
        CompressHostKernels.compress_decode(src, 2, chunk, S, first, 0, g16, g32, layout, want, S)
        for off in (0, 1):
            whole = torch.full((2 * S + off + 4,), 9.0, device=dev)
            out = whole[off:off + 2 * S]
            ops.compress_decode(dsrc, 2, chunk, S, first, 0, dg16, dg32, layout, out, S)
            assert torch.equal(_bits(out), _bits(want)), (first, off)
            assert (whole[:off] == 9.0).all() and (whole[off + 2 * S:] == 9.0).all()
        i = first + np.arange(S)
        assert (want[:S][torch.from_numpy(i > n + (layout != "plain"))] == 0).all()  # beyond the tail: +0
        assert (want[S:].view(torch.int32) == (0x7fc00000 if layout == "robust" else 0)).all()  # the invalid client
    # a whole bucket per call; the valid client's equals what the pack kernels write for the weights g + scale * q
    whole_want, whole_got = torch.zeros(world * S), torch.zeros(world * S, device=dev)
    for slot in (0, 1):
        CompressHostKernels.compress_decode(image.view(-1)[slot * chunk:], world, 2 * chunk, S, 0, S, g16, g32, layout,
                                            whole_want, S)
        ops.compress_decode(dimg.view(-1)[slot * chunk:], world, 2 * chunk, S, 0, S, dg16, dg32, layout, whole_got, S)
        assert torch.equal(_bits(whole_got), _bits(whole_want)), slot
        if slot == 0:
            codes = np.concatenate([image[r, 0, :S].numpy().view(np.int8) for r in range(world)])
            scales = np.concatenate([image[r, 0, S:S + S // 64].numpy().view(F32) for r in range(world)])
            y = torch.from_numpy(host_dequant(_cat(g16, g32), codes, scales))
            w = torch.tensor(weight or 1.0)
            tail = [1.0] if layout == "plain" else [float(w), 1.0]
            ref = torch.cat([y * w if layout == "weighted" else y, torch.tensor(tail)])
            assert torch.equal(_bits(whole_got[:ref.numel()]), _bits(ref)) and not whole_got[ref.numel():].any()


def test_argument_errors(dev):
    """Every error returns before any launch: the outputs keep their bits."""
    from federated_multi_modal_amd import _lib
    P, St = ops._p, ops._s
    S = 256
    chunk = chunk_bytes(S)
    p16, g16 = torch.zeros(8, dtype=torch.float16, device=dev), torch.zeros(8, dtype=torch.float16, device=dev)
    p32, g32 = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    e_in, e_out = torch.zeros(16, device=dev), torch.full((16,), 9.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    image = torch.full((chunk,), SENTINEL, dtype=torch.uint8, device=dev)
    out = torch.full((S,), 9.0, device=dev)

    def q(**kw):
        a = dict(x16=P(p16), g16=P(g16), n16=8, x32=P(p32), g32=P(g32), n32=8, e_in=P(e_in), e_out=P(e_out),
                 flag=P(flag), weight=1.0, rounding=0, seed=1, rnd=0, client=0, image=P(image), stride=chunk, S=S,
                 world=1)
        a.update(kw)
        return tuple(a.values()) + (St(),)

    def d(**kw):
        a = dict(image=P(image), stride=chunk, nclients=1, S=S, first=0, step=0, g16=P(g16), n16=8, g32=P(g32), n32=8,
                 layout=0, out=P(out), ostride=S)
        a.update(kw)
        return tuple(a.values()) + (St(),)

    for name, args, text in (("mf_compress_quantize", q(S=100), "multiple of 256"),
                             ("mf_compress_quantize", q(n16=-1), "negative"),
                             ("mf_compress_quantize", q(rounding=2), "rounding"),
                             ("mf_compress_quantize", q(image=None), "null"),
                             ("mf_compress_quantize", q(e_out=None), "residual"),
                             ("mf_compress_quantize", q(n32=300), "shorter"),
                             ("mf_compress_decode", d(S=100), "multiple of 256"),
                             ("mf_compress_decode", d(layout=3), "layout"),
                             ("mf_compress_decode", d(first=-1), "negative"),
                             ("mf_compress_decode", d(out=None), "null")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert (image == SENTINEL).all() and (out == 9.0).all() and (e_out == 9.0).all()


# ----------------------------------------------------------------------------- FedAvgBucket on the device

# round 0: client 1 returns a NaN; round 1: client 2 fails after it was packed (a re-exchange with the same codes)
SCEN = (((1,), ()), ((), (2,)))


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for c, ((p16, p32, e), (q16, q32, f)) in enumerate(zip(a[1], b[1])):
        assert torch.equal(p16, q16) and torch.equal(p32, q32), c
        assert (e is None and f is None) or torch.equal(_bits(e), _bits(f)), c


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
def test_three_clients_in_one_process_and_over_the_rccl_chain(dev, rccl_group, rounding):  # noqa: F811
    """Two rounds of three clients on the device, decoded locally (one process) and through all_to_all of the uint8
    image -> decode -> reduce -> all_gather on the side stream in a one-rank group: fp16 weights, residuals and
    n_valid equal the host-kernel run of the same scenario bit for bit."""
    host = run_rounds([0, 1, 2], SCEN, rounding=rounding)
    assert host[0] == [2, 2] and all(e.any() for _, _, e in host[1])
    _same(run_rounds([0, 1, 2], SCEN, rounding=rounding, kernels=None, device=dev), host)
    _same(run_rounds([0, 1, 2], SCEN, rounding=rounding, kernels=None, device=dev, shard_single=True), host)


@pytest.mark.parametrize("kw", [dict(weights=(3.0, 1.0, 2.0)), dict(robust="median"), dict(error_feedback=False)])
def test_layouts_over_the_rccl_chain(dev, rccl_group, kw):  # noqa: F811
    _same(run_rounds([0, 1, 2], SCEN, kernels=None, device=dev, shard_single=True, **kw), run_rounds([0, 1, 2], SCEN, **kw))


def test_server_optimizer_consumes_the_decoded_mean(dev, rccl_group):  # noqa: F811
    host = run_rounds([0, 1, 2], SCEN, server="fedadam")
    _same(run_rounds([0, 1, 2], SCEN, server="fedadam", kernels=None, device=dev, shard_single=True), host)
    _same(run_rounds([0, 1, 2], SCEN, server="fedadam", kernels=None, device=dev), host)


# ----------------------------------------------------------------------------- through the trainer

def test_compression_through_the_trainer(dev, tmp_path, capsys):
    """FED.COMPRESS none logs nothing, allocates nothing and keeps the plain exchange's bits (the mean of the two
    clients in client order, rounded to fp16: what a run without the keys computes); FED.COMPRESS int8 logs the
    uplink bytes once and gives the restatement's weights and residuals."""
    off = build_trainer(small_cfg(tmp_path / "off", clients=2, extra=["FED.COMPRESS", "none"]))
    assert "compression" not in capsys.readouterr().out
    on = build_trainer(small_cfg(tmp_path / "on", clients=2, extra=["FED.COMPRESS", "int8"]))
    log = capsys.readouterr().out
    f0 = on.fed[0]
    n = f0.e.n16 + f0.e.n32
    wire, full = on.exchange.world * on.exchange.chunk, 4 * (n + 1)
    assert log.count("[INFO] FedAvg uplink compression int8") == 1
    assert f"{wire} bytes per client and round instead of {full}" in log and "simulated" in log
    assert "residuals are not checkpointed" in log
    assert all(f.compress is None and f.resid is None for f in off.fed) and off.exchange.image is None
    assert all(f.compress == "int8" and f.client == c.client_id for f, c in zip(on.fed, on.clients))
    assert off.fed[0].pbuf.numel() == n + 1 and off.exchange.stage.shape == (1, 2, n + 1)  # the buffers as they were
    res = [np.zeros(n, F32) for _ in on.clients]
    for rnd in (1, 2):
        for tr in (off, on):
            _local_results(tr, rnd)
        rows = [torch.cat([c.engine.flat16.float(), c.engine.flat32]).cpu() for c in off.clients]
        plain = ((rows[0] + rows[1]) / 2.0).half()
        g = _cat(f0.global16.cpu(), f0.global32.cpu())
        acc = None
        for j, c in enumerate(on.clients):
            codes, scales, res[j] = host_quantize(_cat(c.engine.flat16.cpu(), c.engine.flat32.cpu()), g, res[j], False,
                                                  "nearest", on.compress["seed"], rnd - 1, c.client_id, f0.pbuf.numel())
            y = torch.from_numpy(host_dequant(g, codes, scales))
            acc = y if acc is None else acc + y
        want = (acc / 2.0).half()
        assert off._fedavg([]) == 2 and on._fedavg([]) == 2
        for c in off.clients:
            assert torch.equal(c.engine.flat16.cpu(), plain[:f0.e.n16])
            assert torch.equal(c.engine.flat32.cpu(), plain[f0.e.n16:].float())
        assert not _same_weights(off, on)
        for j, c in enumerate(on.clients):
            assert torch.equal(c.engine.flat16.cpu(), want[:f0.e.n16]), (rnd, j)
            assert torch.equal(c.engine.flat32.cpu(), want[f0.e.n16:].float()), (rnd, j)
            assert np.array_equal(on.fed[j].resid.cpu().numpy().view(np.int32), res[j].view(np.int32)), (rnd, j)
    assert on.exchange.round == 2 and res[0].any()
    # a resumed run restarts the residuals at zero, and says so
    on.save_model()
    capsys.readouterr()
    on.load_model(str(tmp_path / "on"), epoch=on.cfg.OPTIM.MAX_EPOCH)
    assert "residuals restart at zero" in capsys.readouterr().out
    assert not any(f.resid.any() for f in on.fed) and on.exchange.round == 2
