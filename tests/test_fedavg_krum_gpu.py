"""GPU tier: Multi-Krum's kernels (mf_krum_pairwise, mf_krum_select, mf_fedavg_reduce_selected) against the host
restatement of tests/_krum_ref.py -- the distances to the derived bound on two summation orders, the selection and the
selected mean bit for bit -- then through FedAvgBucket / FedAvgExchange on the device (one process, and the RCCL chain
in a one-rank group), with the int8 uplink, and through the trainer."""
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

from _krum_ref import gamma2, host_pairwise, host_select, host_selected_mean, stable_selection
from federated_multi_modal_amd import ops
from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange
from federated_multi_modal_amd.trainers import build_trainer
from test_fedavg_compress_dist import run_rounds as compress_rounds
from test_fedavg_robust_gpu import N16, N32, _Eng
from test_fedprox_weighted_gpu import small_cfg

pytestmark = pytest.mark.gpu

NAN = float("nan")
CANARY = -7.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def device_image(x, aligned, dev):
    """x laid out [client][stride] on the device.  aligned: stride % 4 == 0 at a 16-byte aligned base; else the base
    one float past an aligned allocation and an odd stride.  The slack between the rows holds a value that would show
    in any result.  Returns (the flat image, stride)."""
    nclients, n = x.shape
    stride = (n + 7) // 4 * 4 if aligned else (n + 2) | 1
    offset = 0 if aligned else 1
    flat = torch.full((offset + nclients * stride,), 7e4, dtype=torch.float32)
    flat[offset:].view(nclients, stride)[:, :n] = x
    img = flat.to(dev)[offset:]
    assert (img.data_ptr() % 16 == 0) == aligned and (stride % 4 == 0) == aligned
    return img, stride


# ----------------------------------------------------------------------------- the distances

def make_clients(nclients, n, seed, far):
    """[nclients, n] fp32 on the CPU: every client the same weights over twelve binades plus a small update of its
    own (what a Gram matrix would cancel on), two absent clients when there are three or more, and with `far` two
    present clients further apart at one coordinate than the fp32 range.  Returns (x, absent)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 6, (n,), generator=g).float())
    x = base + 1e-3 * torch.randn(nclients, n, generator=g) * (1.0 + base.abs())
    absent = sorted({1, nclients - 1}) if nclients >= 3 else []
    for c in absent:
        x[c] = NAN
    present = [c for c in range(nclients) if c not in absent]
    if far and len(present) >= 2:
        x[present[0], n // 2], x[present[1], n // 2] = 3e38, -3e38
    return x, absent


@pytest.mark.parametrize("nclients", [1, 2, 3, 8, 9, 16, 17, 33, 64])
def test_pairwise_against_the_restatement(dev, nclients):
    """Client counts that straddle the 8-wide pair tile, coordinate counts from 1 to past two chunks, an aligned image
    and one a float off with an odd stride.  The NaN pattern, bitwise symmetry, +0 on the present diagonal, +inf for
    the pair beyond the fp32 range, |got - want| <= 2 gamma_n want (any two orders of n non-negative fp64 terms agree
    to that: derived, not measured), the same bits on a second call, and untouched canaries after dist and ws."""
    chunk = ops.krum_chunk_elems()
    sizes = [1, 3, 255, 4099] + ([chunk + 5, 2 * chunk + 5] if nclients <= 16 else [])
    nn = nclients * nclients
    for n in sizes:
        far = n == 255
        x, absent = make_clients(nclients, n, 31 * nclients + n, far)
        want = host_pairwise(x)
        for aligned in (True, False):
            img, stride = device_image(x, aligned, dev)
            need = ops.krum_ws_bytes(nclients, n)
            assert need % 8 == 0
            ws = torch.full((need // 8 + 8,), CANARY, dtype=torch.float64, device=dev)
            out = torch.full((nn + 8,), CANARY, dtype=torch.float64, device=dev)
            ops.krum_pairwise(img, nclients, n, ws[:need // 8], out[:nn])
            got = out[:nn].cpu().numpy().reshape(nclients, nclients).copy()
            ops.krum_pairwise(img, nclients, n, ws[:need // 8], out[:nn])
            again = out[:nn].cpu().numpy().reshape(nclients, nclients)
            where = (nclients, n, aligned)
            assert (out[nn:] == CANARY).all() and (ws[need // 8:] == CANARY).all(), where
            assert np.array_equal(got.view(np.int64), again.view(np.int64)), where
            assert np.array_equal(got.view(np.int64), got.T.copy().view(np.int64)), where
            assert np.array_equal(np.isnan(got), np.isnan(want)), where
            for c in range(nclients):
                if c in absent:
                    assert np.isnan(got[c]).all() and np.isnan(got[:, c]).all(), where
                else:
                    assert got[c, c] == 0.0 and not np.signbit(got[c, c]), where
            fin = np.isfinite(want)
            assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), where  # +inf
            assert (np.abs(got[fin] - want[fin]) <= gamma2(n) * want[fin]).all(), where
            if far and nclients - len(absent) >= 2:
                assert np.isposinf(got).sum() == 2, where
            if n == 4099 and nclients - len(absent) >= 2:
                assert (got[fin] > 0).sum() >= 2, where
    # no coordinate: the zero matrix
    out = torch.full((nn,), CANARY, dtype=torch.float64, device=dev)
    ws = torch.zeros(ops.krum_ws_bytes(nclients, 0) // 8, dtype=torch.float64, device=dev)
    ops.krum_pairwise(torch.zeros(nclients * 4, device=dev), nclients, 0, ws, out)
    assert (out == 0).all() and not torch.signbit(out).any()


# ----------------------------------------------------------------------------- the selection

def _device_select(parts, nclients, f, m, dev):
    p = torch.from_numpy(np.ascontiguousarray(parts, np.float64)).reshape(-1).to(dev)
    sel = torch.full((nclients,), -5, dtype=torch.int32, device=dev)
    scores = torch.full((nclients,), CANARY, dtype=torch.float64, device=dev)
    counts = torch.full((3,), -5, dtype=torch.int32, device=dev)
    ops.krum_select(p, nclients, f, m, sel, scores, counts)
    return sel.cpu().tolist(), scores.cpu().numpy(), tuple(counts.cpu().tolist())


def _split(D, nparts, rng):
    """nparts non-negative symmetric matrices (the absent clients NaN in each, as every shard sees them); their
    in-order sum is what both sides combine."""
    if nparts == 1:
        return D[None].copy()
    w = rng.uniform(0.1, 1.0, (nparts,) + D.shape)
    w = np.triu(w) + np.transpose(np.triu(w, 1), (0, 2, 1))
    with np.errstate(invalid="ignore"):
        return w * D[None]


def _crafted(p, kind, rng):
    """A distance matrix with p present clients and absent ones interleaved (none at p = 64).  kind "real": random
    points; "ties": integer points on a line, so many scores tie exactly, and one pair at +inf."""
    nclients = 64 if p == 64 else 2 * p + 3
    present = list(range(64)) if p == 64 else [2 * k + 1 for k in range(p)]
    if kind == "real":
        pts = torch.from_numpy(rng.normal(size=(nclients, 5)).astype(np.float32))
    else:
        pts = torch.from_numpy(rng.integers(0, 6, size=(nclients, 1)).astype(np.float32))
    for c in range(nclients):
        if c not in present:
            pts[c] = NAN
    D = host_pairwise(pts)
    if kind == "ties" and p >= 2:
        a, b = present[0], present[-1]
        D[a, b] = D[b, a] = np.inf
    return nclients, D


@pytest.mark.parametrize("p", [0, 1, 2, 3, 5, 8, 64])
def test_select_against_the_restatement(dev, p):
    """selected, scores and counts bit for bit, over 1, 2, 3 and 8 parts, f in 0, 1, 2, 40 and m in 0, 1, 3, 100, on
    random distances and on ones with exact score ties and a +inf entry; the scores carry the in-order sum of the
    parts (the scores of the q = 1 settings are single combined entries)."""
    rng = np.random.default_rng(50 + p)
    for kind in ("real", "ties"):
        nclients, D = _crafted(p, kind, rng)
        for nparts in (1, 2, 3, 8):
            parts = _split(D, nparts, rng)
            for f in (0, 1, 2, 40):
                for m in (0, 1, 3, 100):
                    want_sel, want_scores, want_counts, _ = host_select(parts, f, m)
                    sel, scores, counts = _device_select(parts, nclients, f, m, dev)
                    where = (p, kind, nparts, f, m)
                    assert counts == want_counts and counts[0] == p, where
                    assert sel == want_sel and sum(sel) == counts[2], where
                    assert np.array_equal(scores.view(np.int64), want_scores.view(np.int64)), where


def test_select_adds_the_parts_in_order_and_reads_every_entry(dev):
    """Three present clients, f = 0: q = 1, so each score is one combined entry.  The parts 1, 2^-53, 2^-53 give 1 when
    added in order from part 0 and 1 + 2^-52 in any order that adds the small ones first; moving the small entry over
    every pair reads back each combined entry."""
    tiny = 2.0 ** -53
    for i, j in ((0, 1), (0, 2), (1, 2)):
        parts = np.zeros((3, 3, 3))
        parts[0] = 8.0 * (1 - np.eye(3))
        parts[1] = 8.0 * tiny * (1 - np.eye(3))
        parts[2] = 8.0 * tiny * (1 - np.eye(3))
        for k, v in enumerate((1.0, tiny, tiny)):
            parts[k, i, j] = parts[k, j, i] = v
        want_sel, want_scores, want_counts, D = host_select(parts, 0, 1)
        assert D[i, j] == 1.0 and D[i, j] != (tiny + tiny) + 1.0 and want_counts == (3, 0, 1)
        sel, scores, counts = _device_select(parts, 3, 0, 1, dev)
        assert counts == want_counts and sel == want_sel and sel[i] == 1
        assert np.array_equal(scores.view(np.int64), want_scores.view(np.int64)) and scores[i] == 1.0 == scores[j]


def test_worked_example_on_the_device(dev):
    """The 1-D clients 0, 1, 2, 3, 100 with f = 1 through all three kernels: scores 5, 2, 2, 5, 19013; m = 1 keeps
    client 1, m = 3 gives the mean 1.0, m = 0 the mean 1.5."""
    x = torch.tensor([0.0, 1.0, 2.0, 3.0, 100.0]).view(5, 1)
    img = x.to(dev).view(-1)
    ws = torch.zeros(ops.krum_ws_bytes(5, 1) // 8, dtype=torch.float64, device=dev)
    D = torch.zeros(25, dtype=torch.float64, device=dev)
    ops.krum_pairwise(img, 5, 1, ws, D)
    assert np.array_equal(D.cpu().numpy().reshape(5, 5), host_pairwise(x))
    sel = torch.zeros(5, dtype=torch.int32, device=dev)
    scores = torch.zeros(5, dtype=torch.float64, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    out = torch.zeros(1, device=dev)
    for m, want_sel, want_mean in ((1, [0, 1, 0, 0, 0], 1.0), (3, [1, 1, 1, 0, 0], 1.0), (0, [1, 1, 1, 1, 0], 1.5)):
        ops.krum_select(D, 5, 1, m, sel, scores, counts)
        ops.fedavg_reduce_selected(img, 5, sel, -1, out)
        assert sel.tolist() == want_sel and scores.tolist() == [5.0, 2.0, 2.0, 5.0, 19013.0]
        assert counts.tolist() == [5, 1, sum(want_sel)] and out.item() == want_mean


# ----------------------------------------------------------------------------- the selected mean

def _masks(nclients):
    return {"none": [0] * nclients, "one": [int(c == nclients // 2) for c in range(nclients)],
            "all": [1] * nclients, "alternating": [c % 2 for c in range(nclients)],
            "last": [int(c == nclients - 1) for c in range(nclients)]}


@pytest.mark.parametrize("nclients", [1, 2, 3, 8, 17, 64])
def test_reduce_selected_against_the_restatement(dev, nclients):
    """Bit for bit: nobody, one, all, every second and only the last client selected; whole rows of NaN in unselected
    clients, which must not leak; the count element inside the range (in the 16-byte part and in the ragged tail) and
    absent; both alignments."""
    n = 1031
    g = torch.Generator().manual_seed(900 + nclients)
    base = torch.randn(nclients, n, generator=g) * torch.exp2(torch.randint(-6, 6, (nclients, n), generator=g).float())
    for name, mask in _masks(nclients).items():
        x = base.clone()
        x[:, 5] = -0.0
        unselected = [c for c in range(nclients) if not mask[c]]
        for c in unselected[::2]:
            x[c] = NAN
        for aligned in (True, False):
            img, _ = device_image(x, aligned, dev)
            sel = torch.tensor(mask, dtype=torch.int32, device=dev)
            for count_pos in (-1, 2, n - 1):
                want = host_selected_mean(x, mask, count_pos)
                buf = torch.full((n + 12,), 3e4, device=dev)
                out = buf[4:4 + n] if aligned else buf[5:5 + n]
                ops.fedavg_reduce_selected(img, nclients, sel, count_pos, out)
                where = (nclients, name, aligned, count_pos)
                assert torch.equal(_bits(out), _bits(want)), where
                assert not torch.isnan(out).any(), where
                assert (buf[:4] == 3e4).all() and (buf[5 + n:] == 3e4).all(), where
                if count_pos >= 0:
                    assert out[count_pos].item() == nclients - len(unselected[::2]), where


# ----------------------------------------------------------------------------- FedAvgBucket on the device

F = 1


def _five_clients(dev, invalid=(), **kw):
    """Five buckets built on the global weights (engine seed 0), then each engine given its local result; client 2 is
    far off, and finite."""
    engines, feds = [], []
    for c in range(5):
        e = _Eng(dev, 0)
        feds.append(FedAvgBucket(e, robust="multi_krum", krum_f=F, shard_single=dist.is_initialized(), **kw))
        loc = _Eng(dev, 10 + c, scale=-50.0 if c == 2 else 1.0)
        e.flat16.copy_(loc.flat16)
        e.flat32.copy_(loc.flat32)
        if c in invalid:
            e.flat32[7] = NAN
        engines.append(e)
    return engines, feds


def _host_bucket(engines, invalid=()):
    """(the restatement's selection, its bucket [statistic | 1 | p]); the selection's stability is asserted first."""
    rows = []
    for c, e in enumerate(engines):
        row = torch.cat([e.flat16.float().cpu(), e.flat32.cpu(), torch.ones(2)])
        rows.append(torch.full_like(row, NAN) if c in invalid else row)
    g = torch.stack(rows)
    sel = stable_selection(host_pairwise(g), F, 0)
    return sel, host_selected_mean(g, sel, N16 + N32 + 1)


def _exchange(feds):
    x = FedAvgExchange(feds, robust="multi_krum", krum_f=F, shard_single=dist.is_initialized())
    for fed in feds:
        fed.pack()
    x.start()
    x.finish()
    stat = feds[0].buf.clone()
    for fed in feds:
        fed.unpack()
    torch.cuda.synchronize()
    return x, stat


def _check_round(dev, invalid):
    engines, feds = _five_clients(dev, invalid)
    sel, want = _host_bucket(engines, invalid)
    x, stat = _exchange(feds)
    n = N16 + N32
    p = 5 - len(invalid)
    kept, scores, got_p, fe, me = x.krum_stats()
    assert x.n_valid() == p == got_p and float(want[n]) == 1.0 and float(want[n + 1]) == p
    assert kept == [c for c in range(5) if sel[c]] and me == len(kept) == p - fe
    assert 2 not in kept or p < 5  # the outlier is dropped while f = 1 can be carried
    assert fe == (1 if p >= 5 else 0) and [s != s for s in scores] == [c in invalid for c in range(5)]
    assert torch.equal(_bits(stat), _bits(want))
    val = want[:n].half()
    for e in engines:
        assert e.loaded == 1
        assert torch.equal(e.flat16.cpu(), val[:N16]) and torch.equal(e.flat32.cpu(), val[N16:].float())
    return x, sel


def _nobody_and_single(dev):
    engines, feds = _five_clients(dev, (0, 1, 2, 3, 4))
    glob = _Eng(dev, 0)
    x, _ = _exchange(feds)
    assert x.n_valid() == 0 and x.krum_stats()[0] == []
    for e in engines:
        assert torch.equal(e.flat16, glob.flat16) and torch.equal(e.flat32, glob.flat32)
    # a single client: kept when valid; invalid, its absence marks become a zero vote and the global copy comes back
    e = _Eng(dev, 0)
    fed = FedAvgBucket(e, robust="multi_krum", krum_f=F, shard_single=dist.is_initialized())
    g16, g32 = e.flat16.clone(), e.flat32.clone()
    e.flat32.mul_(2.0)
    assert fed.run() == 1 and torch.equal(e.flat32, (g32 * 2).half().float())
    assert fed.exchange.krum_stats()[0] == [0]
    e.flat16[3] = NAN
    assert fed.run() == 0
    assert torch.equal(e.flat16, g16) and torch.equal(e.flat32, (g32 * 2).half().float())


def test_five_clients_in_one_process(dev):
    """The bucket reads [mean of the four | 1.0 | 5], bit-equal to the restatement, and the outlier is dropped; with
    an invalid client p = 4, where f degrades to 0 and all four present clients are kept, as the restatement keeps
    them; nobody valid returns the global copy; a single client runs."""
    assert not dist.is_initialized()
    x, sel = _check_round(dev, ())
    assert sel == [1, 1, 0, 1, 1] and not x.distributed and x.local_stage is not None
    _, sel = _check_round(dev, (0,))
    assert sel == [0, 1, 1, 1, 1]
    _nobody_and_single(dev)


@pytest.fixture
def rccl_group(dev):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    yield
    dist.destroy_process_group()


INT8_SCEN = (((1,), ()), ((), ()))  # round 0: client 1 invalid; round 1: everybody


def _same(a, b):
    assert a[0] == b[0]
    for (a16, a32, ar), (b16, b32, br) in zip(a[1], b[1]):
        assert torch.equal(a16, b16) and torch.equal(a32, b32) and torch.equal(_bits(ar), _bits(br))


def test_five_clients_over_the_rccl_chain(dev, rccl_group):
    """all_to_all -> mf_krum_pairwise -> all_gather of the parts -> mf_krum_select -> mf_fedavg_reduce_selected ->
    all_gather on the side stream in a one-rank group (shard_single); then two int8 rounds under Multi-Krum over the
    chain against the same rounds in one process (the distances run over the same n, stride and chunks either way,
    so their bits, and the selection, are the same)."""
    x, sel = _check_round(dev, ())
    assert sel == [1, 1, 0, 1, 1] and x.sharded and x.side is not None and 0 <= x.count_pos < x.S
    _check_round(dev, (2,))
    _nobody_and_single(dev)
    ids = [0, 1, 2, 3, 4]
    chain = compress_rounds(ids, INT8_SCEN, robust="multi_krum", kernels=None, device=dev, shard_single=True)
    assert chain[0] == [4, 5]
    # without shard_single a one-rank group is not distributed: the one-process path
    _same(chain, compress_rounds(ids, INT8_SCEN, robust="multi_krum", kernels=None, device=dev))


# ----------------------------------------------------------------------------- through the trainer

def _snap(c):
    return {n: c.engine.P[n].detach().clone().cpu() for n in c.engine.trainable_names}


def test_krum_round_through_the_trainer(dev, tmp_path, capsys):
    """FED.KRUM_F 0, FED.KRUM_M 1 with three clients is Krum: after the round every client holds fp16 of exactly one
    client's snapshot, the one the restatement selects from the snapshots."""
    extra = ["FED.ROBUST_AGG", "multi_krum", "FED.KRUM_F", 0, "FED.KRUM_M", 1]
    tr = build_trainer(small_cfg(tmp_path, clients=3, extra=extra))
    assert "[INFO] Robust aggregation: Multi-Krum" in capsys.readouterr().out
    assert all(f.robust == "multi_krum" and (f.krum_f, f.krum_m) == (0, 1) for f in tr.fed) and tr.exchange.krum
    for c in tr.clients:
        c.run_epoch(0)
    snaps = [_snap(c) for c in tr.clients]
    assert not all(torch.equal(snaps[0][n], snaps[1][n]) for n in snaps[0])
    rows = torch.stack([torch.cat([s[n].float().reshape(-1) for n in sorted(s)]) for s in snaps])
    sel = stable_selection(host_pairwise(rows), 0, 1)  # the precondition
    assert sum(sel) == 1
    k = sel.index(1)
    capsys.readouterr()
    assert tr._fedavg([]) == 3
    log = capsys.readouterr().out
    assert f"[Round 1] Multi-Krum: kept clients [{k}] of 3 present, scores " in log
    assert tr.exchange.krum_stats()[0] == [k] and tr.exchange.krum_stats()[2:] == (3, 0, 1)
    for name in snaps[0]:
        want = snaps[k][name].float().half().float()
        for c in tr.clients:
            assert torch.equal(c.engine.P[name].detach().cpu().float(), want), name
    with pytest.raises(ValueError, match="FED.NUM_CLIENTS"):
        build_trainer(small_cfg(tmp_path / "bad", clients=3, extra=["FED.ROBUST_AGG", "multi_krum", "FED.KRUM_F", 1]))
