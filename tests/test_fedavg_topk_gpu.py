"""GPU tier: the top-k uplink kernels (mf_topk_select, mf_topk_decode) against the numpy fp32 restatement of
tests/test_fedavg_topk_dist.py, bit for bit -- values, indices, padding bytes, tail and residual -- then through
FedAvgBucket / FedAvgExchange on the device (one process, and the RCCL chain in a one-rank group), with a server
optimizer, and through the trainer."""
import numpy as np
import pytest
import torch

from federated_multi_modal_amd import ops
from federated_multi_modal_amd.trainers import build_trainer
from test_fedavg_compress_dist import B, F32, _cat
from test_fedavg_compress_gpu import SENTINEL, SHAPES, _at, _bits, _inputs, _same
from test_fedavg_dp_gpu import _local_results, rccl_group  # noqa: F401  (rccl_group: a fixture)
from test_fedavg_topk_dist import TopkHostKernels, host_dense, host_select, run_rounds, scatter, topk_chunk_bytes, wire
from test_fedprox_weighted_gpu import small_cfg

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 64)


def _topk_inputs(n16, n32):
    """The int8 test's inputs (block 0 all zero, block 1 one large value among small ones) and, where there are four
    blocks, block 2 full of ties (four values of magnitude 1 at 7, 8, 9 and 200, the rest five small magnitudes that
    repeat) and block 3 all of one magnitude with alternating signs: g = 0 and e = 0 there and x exact in fp16, so
    u = x whichever buffer a coordinate lies in.  At (1000, 777) block 3 straddles the fp16 / fp32 boundary.  No u is
    subnormal."""
    x16, g16, x32, g32, e = _inputs(n16, n32)
    n = n16 + n32
    if n >= 4 * B:
        x, g = torch.cat([x16.float(), x32]), torch.cat([g16.float(), g32])
        j = torch.arange(B)
        tie = ((j % 5 + 1).float() * 2.0 ** -10) * torch.where(j % 3 == 0, -1.0, 1.0)
        tie[7], tie[8], tie[9], tie[200] = 1.0, -1.0, 1.0, -1.0
        x[2 * B:3 * B] = tie
        x[3 * B:4 * B] = torch.where(j % 2 == 0, 0.25, -0.25)
        g[2 * B:4 * B] = 0.0
        e[2 * B:4 * B] = 0.0
        x16, x32, g16, g32 = x[:n16].half(), x[n16:].clone(), g[:n16].half(), g[n16:].clone()
        assert torch.equal(x16.float(), x[:n16])
    return x16, g16, x32, g32, e.contiguous()


@pytest.mark.parametrize("n16,n32", SHAPES)
def test_select_matches_the_host_restatement(dev, n16, n32):
    """Values, indices, padding bytes, tail and e' bit for bit: k = 1, 3, 8 and 64; the buffers 16-byte aligned, all one
    element off (element accesses throughout) and mixed; S for one destination rank and for three; with and without a
    residual; a valid client and one with the validity flag set (every value and index byte zero, weight and vote 0,
    e' = e); the other slot of the image and everything around e' untouched, e never written."""
    cpu = _topk_inputs(n16, n32)
    x16, g16, x32, g32, e = cpu
    n = n16 + n32
    x, g = _cat(x16, x32), _cat(g16, g32)
    for world in (1, 3):
        padded = -(-(n + 1) // (world * B)) * world * B
        S = padded // world
        nbk_all = padded // B
        for k in KS:
            chunk = topk_chunk_bytes(S, k)
            assert ops.topk_chunk_bytes(S, k) == chunk
            nbk = S // B * k
            ref = {fb: host_select(x, g, e.numpy() if fb else None, False, k, padded) for fb in (True, False)}
            for offs in ((0,) * 6, (1,) * 6, (1, 0, 0, 1, 1, 0)):
                for feedback, bad, weight in ((True, False, None), (False, False, 2.5), (True, True, 2.5)):
                    d16, dg16, d32, dg32, de = (_at(t, o, dev) for t, o in zip(cpu, offs))
                    whole = torch.full((n + offs[5] + 8,), 77.0, device=dev)
                    e_out = whole[offs[5]:offs[5] + n]
                    flag = torch.full((1,), int(bad), dtype=torch.int32, device=dev)
                    image = torch.full((world, 2, chunk), SENTINEL, dtype=torch.uint8, device=dev)
                    ops.topk_select(d16, d32, dg16, dg32, de if feedback else None, e_out if feedback else None, flag,
                                    weight, k, image, 1, S)
                    if bad:
                        idx, vals, en = host_select(x, g, e.numpy(), True, k, padded)
                    else:
                        idx, vals, en = ref[feedback]
                    want = wire(idx, vals, 0.0 if bad else (weight or 1.0), 0.0 if bad else 1.0, world, S, k)
                    got = image.cpu().numpy()
                    where = (world, k, offs, feedback, bad)
                    assert np.array_equal(got[:, 1, :4 * nbk], want[:, :4 * nbk]), ("values",) + where
                    assert np.array_equal(got[:, 1, 4 * nbk:5 * nbk], want[:, 4 * nbk:5 * nbk]), ("indices",) + where
                    assert not got[:, 1, 5 * nbk:-8].any() and got[:, 1, 5 * nbk:-8].shape[1] == -nbk % 4, where
                    assert np.array_equal(got[:, 1, -8:], want[:, -8:]), ("tail",) + where
                    assert (got[:, 0] == SENTINEL).all(), where
                    out = whole.cpu()
                    if feedback:
                        assert np.array_equal(out[offs[5]:offs[5] + n].numpy().view(np.int32), en.view(np.int32)), where
                        assert (out[:offs[5]] == 77.0).all() and (out[offs[5] + n:] == 77.0).all(), where
                        if bad:
                            assert np.array_equal(en, e.numpy()) and not got[:, 1, :-8].any()
                    else:
                        assert (out == 77.0).all(), where
                    assert torch.equal(de.cpu(), e)  # the residual read is never written
            # what the restatement itself says about these inputs
            idx, vals, en = ref[True]
            assert idx.shape == (nbk_all, k) and idx[-1].tolist()[-k:] == sorted(idx[-1].tolist())
            if n >= 4 * B:
                assert idx[0].tolist() == list(range(k)) and not vals[0].any()        # the all-zero block
                assert (B + 9) % B in idx[1].tolist()                                 # its one large value
                assert set([7, 8, 9][:min(k, 3)]) <= set(idx[2].tolist()) and (k < 4 or 200 in idx[2].tolist())
                assert idx[3].tolist() == list(range(k))                              # the all-equal block
            if n <= padded - B:
                assert idx[-1].tolist() == list(range(k)) and not vals[-1].any()      # a block past n


@pytest.mark.parametrize("layout,weight", (("plain", None), ("weighted", 2.5)))
def test_decode_matches_the_host_restatement(dev, layout, weight):
    """A valid and an invalid client's chunks for four destination ranks of 512 coordinates, n = 1777, k = 1, 3, 8 and
    64: every shard of the received image (the tail elements n and n + 1 outside, inside), shards placed so that n or
    n + 1 is the first or the last element or just outside, a 16-byte aligned out and one a float off, and a whole
    bucket in one call (first_step = S, the local decode)."""
    n16, n32, S, world = 1000, 777, 512, 4
    n = n16 + n32
    x16, g16, x32, g32, e = _topk_inputs(n16, n32)
    dg16, dg32 = g16.to(dev), g32.to(dev)
    for k in KS:
        chunk = topk_chunk_bytes(S, k)
        image = torch.zeros(world, 2, chunk, dtype=torch.uint8)
        for slot, bad in ((0, False), (1, True)):
            TopkHostKernels.topk_select(x16, x32, g16, g32, None, None, torch.tensor([int(bad)], dtype=torch.int32),
                                        weight, k, image, slot, S)
        dimg = image.to(dev)
        firsts = [r * S for r in range(world)] + [n - S + 1, n - S + 2, n - S, n - 1, n, n + 1, n + 2, 3]
        for first in firsts:
            rank = min(first // S, world - 1)  # any chunk serves: the position decides what is written
            src, dsrc = image[rank].reshape(-1), dimg[rank].reshape(-1)
            want = torch.full((2 * S,), 9.0)
            TopkHostKernels.topk_decode(src, 2, chunk, S, first, 0, g16, g32, layout, want, S, k)
            for off in (0, 1):
                whole = torch.full((2 * S + off + 4,), 9.0, device=dev)
                out = whole[off:off + 2 * S]
                ops.topk_decode(dsrc, 2, chunk, S, first, 0, dg16, dg32, layout, out, S, k)
                assert torch.equal(_bits(out), _bits(want)), (k, first, off)
                assert (whole[:off] == 9.0).all() and (whole[off + 2 * S:] == 9.0).all()
            i = first + np.arange(S)
            assert (want[:S][torch.from_numpy(i > n + (layout != "plain"))] == 0).all()  # beyond the tail: +0
            assert not want[S:].view(torch.int32).any()                                  # the invalid client: +0
        # a whole bucket per call; the valid client's equals what the pack kernels write for the weights g + s
        whole_want, whole_got = torch.zeros(world * S), torch.zeros(world * S, device=dev)
        for slot in (0, 1):
            TopkHostKernels.topk_decode(image.view(-1)[slot * chunk:], world, 2 * chunk, S, 0, S, g16, g32, layout,
                                        whole_want, S, k)
            ops.topk_decode(dimg.view(-1)[slot * chunk:], world, 2 * chunk, S, 0, S, dg16, dg32, layout, whole_got, S, k)
            assert torch.equal(_bits(whole_got), _bits(whole_want)), (k, slot)
            if slot == 0:
                idx, vals, _ = host_select(_cat(x16, x32), _cat(g16, g32), None, False, k, world * S)
                y = torch.from_numpy(host_dense(_cat(g16, g32), idx, vals))
                w = torch.tensor(weight or 1.0)
                tail = [1.0] if layout == "plain" else [float(w), 1.0]
                ref = torch.cat([y * w if layout == "weighted" else y, torch.tensor(tail)])
                assert torch.equal(_bits(whole_got[:ref.numel()]), _bits(ref)) and not whole_got[ref.numel():].any()


def test_decode_of_a_malformed_image_stays_inside_its_block(dev):
    """Random index bytes, repeats included, every value the same: whichever entry wins, a named coordinate receives
    that value and no other coordinate anything; nothing outside `out` is written."""
    n16, n32, S, k = 300, 200, 512, 8
    g16, g32 = torch.zeros(n16, dtype=torch.float16), torch.zeros(n32)
    chunk = topk_chunk_bytes(S, k)
    gen = np.random.default_rng(5)
    idx = gen.integers(0, 256, (S // B, k)).astype(np.uint8)
    idx[0] = 255
    idx[1, :4] = 0
    raw = wire(idx, np.full((S // B, k), 3.0, F32), 1.0, 1.0, 1, S, k)[0]
    assert raw.size == chunk
    whole = torch.full((S + 8,), 9.0, device=dev)
    ops.topk_decode(torch.from_numpy(raw).to(dev), 1, chunk, S, 0, 0, g16.to(dev), g32.to(dev), "plain", whole[4:4 + S], S,
                    k)
    want = scatter(idx, np.full((S // B, k), 3.0, F32))
    want[n16 + n32:] = 0.0  # a named coordinate past n receives nothing
    want[n16 + n32] = 1.0   # the vote
    assert np.array_equal(whole[4:4 + S].cpu().numpy(), want)
    assert (whole[:4] == 9.0).all() and (whole[4 + S:] == 9.0).all()


def test_argument_errors(dev):
    """Every error returns before any launch: the outputs keep their bits."""
    from federated_multi_modal_amd import _lib
    P, St = ops._p, ops._s
    S, k = 256, 8
    chunk = topk_chunk_bytes(S, k)
    p16, g16 = torch.zeros(8, dtype=torch.float16, device=dev), torch.zeros(8, dtype=torch.float16, device=dev)
    p32, g32 = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    e_in, e_out = torch.zeros(16, device=dev), torch.full((16,), 9.0, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    image = torch.full((chunk,), SENTINEL, dtype=torch.uint8, device=dev)
    out = torch.full((S,), 9.0, device=dev)

    def q(**kw):
        a = dict(x16=P(p16), g16=P(g16), n16=8, x32=P(p32), g32=P(g32), n32=8, e_in=P(e_in), e_out=P(e_out),
                 flag=P(flag), weight=1.0, k=k, image=P(image), stride=chunk, S=S, world=1)
        a.update(kw)
        return tuple(a.values()) + (St(),)

    def d(**kw):
        a = dict(image=P(image), stride=chunk, nclients=1, S=S, first=0, step=0, g16=P(g16), n16=8, g32=P(g32), n32=8,
                 layout=0, out=P(out), ostride=S, k=k)
        a.update(kw)
        return tuple(a.values()) + (St(),)

    for name, args, text in (("mf_topk_select", q(S=100), "multiple of 256"),
                             ("mf_topk_select", q(n16=-1), "negative"),
                             ("mf_topk_select", q(k=0), "k outside"),
                             ("mf_topk_select", q(k=65), "k outside"),
                             ("mf_topk_select", q(image=None), "null"),
                             ("mf_topk_select", q(e_out=None), "residual"),
                             ("mf_topk_select", q(n32=300), "shorter"),
                             ("mf_topk_decode", d(S=100), "multiple of 256"),
                             ("mf_topk_decode", d(layout=2), "layout"),
                             ("mf_topk_decode", d(k=65), "k outside"),
                             ("mf_topk_decode", d(first=-1), "negative"),
                             ("mf_topk_decode", d(out=None), "null")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert (image == SENTINEL).all() and (out == 9.0).all() and (e_out == 9.0).all()


# ----------------------------------------------------------------------------- FedAvgBucket on the device

# round 0: client 1 returns a NaN; round 1: client 2 fails after it was packed (a re-exchange with the same entries)
SCEN = (((1,), ()), ((), (2,)))


@pytest.mark.parametrize("kw", [dict(), dict(k=3), dict(weights=(3.0, 1.0, 2.0)), dict(error_feedback=False)])
def test_three_clients_in_one_process_and_over_the_rccl_chain(dev, rccl_group, kw):  # noqa: F811
    """Two rounds of three clients on the device, decoded locally (one process) and through all_to_all of the uint8
    image -> decode -> reduce -> all_gather on the side stream in a one-rank group: fp16 weights, residuals and
    n_valid equal the host-kernel run of the same scenario, the CPU tier's result, bit for bit."""
    host = run_rounds([0, 1, 2], SCEN, **kw)
    assert host[0] == [2, 2] and all(e is None or e.any() for _, _, e in host[1])
    _same(run_rounds([0, 1, 2], SCEN, kernels=None, device=dev, **kw), host)
    _same(run_rounds([0, 1, 2], SCEN, kernels=None, device=dev, shard_single=True, **kw), host)


def test_server_optimizer_consumes_the_decoded_mean(dev, rccl_group):  # noqa: F811
    host = run_rounds([0, 1, 2], SCEN, server="fedadam")
    _same(run_rounds([0, 1, 2], SCEN, server="fedadam", kernels=None, device=dev, shard_single=True), host)
    _same(run_rounds([0, 1, 2], SCEN, server="fedadam", kernels=None, device=dev), host)


# ----------------------------------------------------------------------------- through the trainer

def test_sparsification_through_the_trainer(dev, tmp_path, capsys):
    """FED.COMPRESS topk logs the uplink bytes once and gives the restatement's weights and residuals, not the plain
    mean (which tests/test_fedavg_compress_gpu.py pins for the run without the key)."""
    on = build_trainer(small_cfg(tmp_path / "on", clients=2, extra=["FED.COMPRESS", "topk", "FED.COMPRESS_TOPK", 4]))
    log = capsys.readouterr().out
    f0 = on.fed[0]
    n = f0.e.n16 + f0.e.n32
    wire_bytes, full = on.exchange.world * on.exchange.chunk, 4 * (n + 1)
    assert on.exchange.chunk == topk_chunk_bytes(on.exchange.S, 4) and on.compress["k"] == 4
    assert log.count("[INFO] FedAvg uplink compression topk (k = 4 of 256, error feedback)") == 1
    assert f"{wire_bytes} bytes per client and round instead of {full}" in log and "simulated" in log
    assert "residuals are not checkpointed" in log
    assert all(f.compress == "topk" and f.compress_k == 4 and f.client == c.client_id
               for f, c in zip(on.fed, on.clients))
    res = [np.zeros(n, F32) for _ in on.clients]
    for rnd in (1, 2):
        _local_results(on, rnd)
        rows = [torch.cat([c.engine.flat16.float(), c.engine.flat32]).cpu() for c in on.clients]
        plain = ((rows[0] + rows[1]) / 2.0).half()
        g = _cat(f0.global16.cpu(), f0.global32.cpu())
        acc = None
        for j, row in enumerate(rows):
            idx, vals, res[j] = host_select(row.numpy(), g, res[j], False, 4, f0.pbuf.numel())
            y = torch.from_numpy(host_dense(g, idx, vals))
            acc = y if acc is None else acc + y
        want = (acc / 2.0).half()
        assert not torch.equal(want, plain)
        assert on._fedavg([]) == 2
        for j, c in enumerate(on.clients):
            assert torch.equal(c.engine.flat16.cpu(), want[:f0.e.n16]), (rnd, j)
            assert torch.equal(c.engine.flat32.cpu(), want[f0.e.n16:].float()), (rnd, j)
            assert np.array_equal(on.fed[j].resid.cpu().numpy().view(np.int32), res[j].view(np.int32)), (rnd, j)
    assert on.exchange.round == 2 and res[0].any()
