"""GPU tier: the robust aggregation kernels (mf_fedavg_reduce_trimmed, mf_fedavg_pack_robust) against the host
restatement of tests/test_fedavg_robust_dist.py, fp32 output bit for bit -- at trim 0 the statistic differs from the
client-order mean in about 1 % of the fp32 results and in none after the fp16 rounding, so the fp16 weights alone would
not pin the summation order -- then through FedAvgBucket / FedAvgExchange on the device (one process, and the RCCL
chain in a one-rank group), with a server optimizer, and through the trainer."""
import socket

import pytest
import torch
import torch.distributed as dist

from federated_multi_modal_amd import _lib, ops
from federated_multi_modal_amd.federated import FedAvgBucket, FedAvgExchange, ServerOptimizer
from federated_multi_modal_amd.trainers import build_trainer
from test_fedavg_robust_dist import MEDIAN_TRIM, QNAN_BITS, host_trimmed
from test_fedopt_dist import HP, _f, host_step
from test_fedprox_weighted_gpu import small_cfg

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def make_clients(nclients, n, seed):
    """[nclients, n] fp32 on the CPU: fp16-representable values over twelve binades (no fp32 denormal can arise: every
    sum is a multiple of 2^-24), with the planted columns of the contract's corner cases."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(nclients, n, generator=g) * torch.exp2(torch.randint(-6, 6, (nclients, n), generator=g).float()))
    x = x.half().float()
    last, second = nclients - 1, min(1, nclients - 1)
    x[torch.rand(nclients, n, generator=g) < 0.08] = NAN      # single absent cells scattered per coordinate
    x[:, 0] = 1.5                                              # all equal
    x[:, 1] = 0.0
    x[::2, 1] = -0.0                                           # mixed +-0
    x[:, 2] = -0.0                                             # all -0
    x[:, 3] = 2.0
    x[:(nclients + 1) // 2, 3] = 1.0                           # ties across the trim boundary
    x[:, 4] = NAN                                              # every client absent
    x[:, 5] = torch.arange(nclients, dtype=torch.float32) - 3.0
    x[last, 5] = float("inf")                                  # one +Inf
    x[:, 6] = torch.arange(nclients, 0, -1, dtype=torch.float32)
    x.view(torch.int32)[second, 6] = -0x003FFFFF               # 0xffc00001: a NaN with the sign bit set
    x[:, 7] = 0.25
    x[last, 7] = -0.0                                          # a lone -0 among equal values
    if nclients >= 3:
        x[1, 8:] = NAN                                         # a whole client row absent (past the planted columns)
    return x


def device_image(x, stride, offset, dev):
    """x laid out [client][stride] on the device, the base `offset` floats past an aligned allocation; the slack
    between the rows holds a value that would show in any result."""
    nclients, n = x.shape
    flat = torch.full((offset + nclients * stride,), 7e4, dtype=torch.float32)
    flat[offset:].view(nclients, stride)[:, :n] = x
    return flat.to(dev)[offset:]


@pytest.mark.parametrize("nclients", [1, 2, 3, 5, 8, 9, 16, 17, 33, 64])
def test_trimmed_reduce_equals_the_host_restatement(dev, nclients):
    """Each network size and both sides of each boundary; n below one block, a multiple of 4 and ragged; stride n and
    n + 5 (16-byte loads impossible); a base one float off alignment; every trim and count position."""
    for n in (37, 4096, 4099):
        x = make_clients(nclients, n, 10 * nclients + n % 7)
        m = (~torch.isnan(x)).sum(0).float()
        images = [(stride, off, device_image(x, stride, off, dev)) for stride in (n, n + 5) for off in (0, 1)]
        for trim_k in sorted({0, 1, 2, (nclients - 1) // 2, 1000}):
            ref = host_trimmed(x, trim_k)
            for count_pos in (-1, 0, n - 1, n // 2 + 1):
                want = ref.clone()
                if count_pos >= 0:
                    want[count_pos] = m[count_pos]
                for stride, off, img in images:
                    out = torch.full((n + 1,), 9e4, device=dev)[off:off + n]
                    ops.fedavg_reduce_trimmed(img, nclients, trim_k, count_pos, out)
                    bad = (_bits(out) != _bits(want)).nonzero().flatten().tolist()
                    assert not bad, (n, trim_k, count_pos, stride, off, bad[:8], out[bad[:8]].tolist(),
                                     want[bad[:8]].tolist())
    assert torch.equal(_bits(host_trimmed(x, MEDIAN_TRIM)), _bits(host_trimmed(x, (nclients - 1) // 2)))


def test_argument_errors(dev):
    g, out = torch.zeros(65 * 8, device=dev), torch.zeros(8, device=dev)
    P, S = ops._p, ops._s
    for args, text in (((P(g), 65, 8, 8, 0, -1, P(out), S()), "nclients"),
                       ((P(g), 3, 8, 8, -1, -1, P(out), S()), "trim_k"),
                       ((P(g), 3, 8, 8, 0, 8, P(out), S()), "count_pos"),
                       ((P(g), 3, 7, 8, 0, -1, P(out), S()), "stride")):
        with pytest.raises(_lib.MapfedError, match=text):
            _lib.call("mf_fedavg_reduce_trimmed", *args)
    with pytest.raises(ValueError, match="nclients"):
        ops.fedavg_reduce_trimmed(g, 65, 0, -1, out)
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("n16,n32", [(37, 4099), (0, 5), (4096, 0)])
def test_pack_robust(dev, n16, n32):
    g = torch.Generator().manual_seed(n16 + n32)
    p16 = torch.randn(n16, generator=g).half().to(dev)
    p32 = torch.randn(n32, generator=g).to(dev)
    if n32:
        p32[0] = -0.0
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    bucket = torch.full((n16 + n32 + 2,), 5.0, device=dev)
    ops.fedavg_pack_robust(p16, p32, flag, bucket)
    want = torch.cat([p16.float(), p32, torch.ones(2, device=dev)])
    assert torch.equal(_bits(bucket), _bits(want))
    flag.fill_(1)
    ops.fedavg_pack_robust(p16, p32, flag, bucket)
    assert (_bits(bucket) == QNAN_BITS).all()
    with pytest.raises(ValueError, match="bucket"):
        ops.fedavg_pack_robust(p16, p32, flag, bucket[:-1])


def test_client_order_does_not_matter(dev):
    x = make_clients(8, 4099, 3)
    perm = torch.randperm(8, generator=torch.Generator().manual_seed(4))
    assert not torch.equal(perm, torch.arange(8))
    for trim_k in (0, 2, MEDIAN_TRIM):
        a, b = torch.empty(4099, device=dev), torch.empty(4099, device=dev)
        ops.fedavg_reduce_trimmed(x.to(dev), 8, trim_k, -1, a)
        ops.fedavg_reduce_trimmed(x[perm].contiguous().to(dev), 8, trim_k, -1, b)
        assert torch.equal(_bits(a), _bits(b))
    # ... which the client-order sum of the plain path does not have: the property is the sorted order's
    y = make_clients(8, 4099, 3)[:, 16:].contiguous()
    y[1] = y[0]  # no absent row
    y = torch.nan_to_num(y, nan=1.0)
    s1, s2 = torch.empty(y.shape[1], device=dev), torch.empty(y.shape[1], device=dev)
    ops.fedavg_reduce_ordered(y.to(dev).view(-1), 8, s1)
    ops.fedavg_reduce_ordered(y[perm].contiguous().to(dev).view(-1), 8, s2)
    assert not torch.equal(_bits(s1), _bits(s2))


def test_two_wrong_clients_of_eight_cannot_leave_the_honest_range(dev):
    g = torch.Generator().manual_seed(5)
    n = 4099
    honest = torch.randn(6, n, generator=g)
    wrong = 6e4 * (torch.randint(0, 2, (2, n), generator=g).float() * 2 - 1)
    x = torch.cat([honest[:3], wrong[:1], honest[3:], wrong[1:]]).to(dev)
    lo, hi = honest.min(0).values.to(dev), honest.max(0).values.to(dev)
    out = torch.empty(n, device=dev)
    for trim_k in (MEDIAN_TRIM, 2):
        ops.fedavg_reduce_trimmed(x.view(-1), 8, trim_k, -1, out)
        assert ((lo <= out) & (out <= hi)).all()
    ops.fedavg_reduce_trimmed(x.view(-1), 8, 0, -1, out)
    assert not ((lo <= out) & (out <= hi)).all()


# ----------------------------------------------------------------------------- FedAvgBucket on the device

N16, N32 = 1003, 7777


class _Eng:
    def __init__(self, dev, seed, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        self.device = dev
        self.n16, self.n32 = N16, N32
        self.flat16 = (torch.randn(N16, generator=g) * 3 * scale).half().to(dev)
        self.flat32 = (torch.randn(N32, generator=g) * 1e-3 * scale).to(dev)
        self.loaded = 0

    def after_weights_loaded(self):
        self.loaded += 1


def _three_clients(dev, robust, trim_k, invalid=(), server_for=None):
    """Three buckets built on the global weights (engine seed 0), then each engine given its local result."""
    engines, feds, server = [], [], None
    for c in range(3):
        e = _Eng(dev, 0)
        if server_for is not None and server is None:
            server = ServerOptimizer(server_for, e, **HP)
        feds.append(FedAvgBucket(e, robust=robust, trim_k=trim_k, shard_single=dist.is_initialized(), server=server))
        loc = _Eng(dev, 10 + c, scale=-50.0 if c == 2 else 1.0)  # client 2 is far off, and finite
        e.flat16.copy_(loc.flat16)
        e.flat32.copy_(loc.flat32)
        if c in invalid:
            e.flat32[7] = NAN
        engines.append(e)
    return engines, feds, server


def _host_bucket(engines, trim, invalid=()):
    rows = []
    for c, e in enumerate(engines):
        row = torch.cat([e.flat16.float().cpu(), e.flat32.cpu(), torch.ones(2)])
        rows.append(torch.full_like(row, NAN) if c in invalid else row)
    return host_trimmed(torch.stack(rows), trim, N16 + N32 + 1)


def _exchange(engines, feds, robust, trim_k):
    x = FedAvgExchange(feds, robust=robust, trim_k=trim_k, shard_single=dist.is_initialized())
    for f in feds:
        f.pack()
    x.start()
    x.finish()
    stat = feds[0].buf.clone()
    for f in feds:
        f.unpack()
    torch.cuda.synchronize()
    return x, stat


def _check_round(dev, robust, trim_k, trim, invalid):
    engines, feds, _ = _three_clients(dev, robust, trim_k, invalid)
    want = _host_bucket(engines, trim, invalid)
    x, stat = _exchange(engines, feds, robust, trim_k)
    n = N16 + N32
    assert x.n_valid() == 3 - len(invalid) and float(want[n]) == 1.0
    assert torch.equal(_bits(stat), _bits(want))
    val = want[:n].half()
    for e in engines:
        assert e.loaded == 1
        assert torch.equal(e.flat16.cpu(), val[:N16]) and torch.equal(e.flat32.cpu(), val[N16:].float())
    return x


@pytest.mark.parametrize("robust,trim_k,trim", [("median", 1, MEDIAN_TRIM), ("trimmed_mean", 1, 1)])
def test_three_clients_in_one_process(dev, robust, trim_k, trim):
    assert not dist.is_initialized()
    x = _check_round(dev, robust, trim_k, trim, ())
    assert not x.distributed and x.local_stage is not None
    _check_round(dev, robust, trim_k, trim, (1,))
    # a single client, invalid: the kernel turns its absence marks into a zero vote and the global copy comes back
    e = _Eng(dev, 0)
    fed = FedAvgBucket(e, robust=robust, trim_k=trim_k)
    g16, g32 = e.flat16.clone(), e.flat32.clone()
    e.flat32.mul_(2.0)
    assert fed.run() == 1 and torch.equal(e.flat32, (g32 * 2).half().float())
    e.flat16[3] = NAN
    assert fed.run() == 0
    assert torch.equal(e.flat16, g16) and torch.equal(e.flat32, (g32 * 2).half().float())


@pytest.fixture
def rccl_group(dev):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    yield
    dist.destroy_process_group()


def test_three_clients_over_the_rccl_chain(dev, rccl_group):
    """all_to_all -> mf_fedavg_reduce_trimmed -> all_gather on the side stream in a one-rank group (shard_single):
    the vote element lies inside the rank's shard, so count_pos is exercised on the sharded path."""
    x = _check_round(dev, "median", 1, MEDIAN_TRIM, ())
    assert x.sharded and x.side is not None and 0 <= x.count_pos < x.S
    _check_round(dev, "trimmed_mean", 1, 1, (0,))
    # nobody valid: the global copy comes back
    engines, feds, _ = _three_clients(dev, "median", 1, (0, 1, 2))
    glob = _Eng(dev, 0)
    x, _ = _exchange(engines, feds, "median", 1)
    assert x.n_valid() == 0
    for e in engines:
        assert torch.equal(e.flat16, glob.flat16) and torch.equal(e.flat32, glob.flat32)
    # with a server optimizer the statistic is the pseudo-gradient's target
    engines, feds, server = _three_clients(dev, "median", 1, (), server_for="fedadam")
    want = _host_bucket(engines, MEDIAN_TRIM)
    x0 = torch.cat([glob.flat16.float(), glob.flat32]).cpu()
    n = N16 + N32
    _exchange(engines, feds, "median", 1)
    tau2 = float(_f(HP["tau"]) * _f(HP["tau"]))
    xs, m, v = host_step("fedadam", want[:n], want[n], x0, torch.zeros_like(x0), torch.full_like(x0, tau2), **HP)
    assert torch.equal(server.x.cpu(), xs) and torch.equal(server.m.cpu(), m) and torch.equal(server.v.cpu(), v)
    val = xs.half()
    for e in engines:
        assert torch.equal(e.flat16.cpu(), val[:N16]) and torch.equal(e.flat32.cpu(), val[N16:].float())
    assert not torch.equal(xs, x0)


# ----------------------------------------------------------------------------- through the trainer

def _snap(c):
    return {n: c.engine.P[n].detach().clone().cpu() for n in c.engine.trainable_names}


def test_median_round_through_the_trainer(dev, tmp_path, capsys):
    tr = build_trainer(small_cfg(tmp_path, clients=3, extra=["FED.ROBUST_AGG", "median"]))
    assert "[INFO] Robust aggregation: coordinate-wise median" in capsys.readouterr().out
    assert all(f.robust == "median" and f.trim == MEDIAN_TRIM for f in tr.fed) and tr.exchange.trim == MEDIAN_TRIM
    for c in tr.clients:
        c.run_epoch(0)
    snaps = [_snap(c) for c in tr.clients]
    assert not all(torch.equal(snaps[0][n], snaps[1][n]) for n in snaps[0])
    assert tr._fedavg([]) == 3
    for name in snaps[0]:
        stack = torch.stack([s[name].float().reshape(-1) for s in snaps])
        want = host_trimmed(stack, MEDIAN_TRIM).half().float().reshape(snaps[0][name].shape)
        for c in tr.clients:
            assert torch.equal(c.engine.P[name].detach().cpu().float(), want), name
    with pytest.raises(ValueError, match="FED.TRIM_K"):
        build_trainer(small_cfg(tmp_path / "bad", clients=2, extra=["FED.ROBUST_AGG", "trimmed_mean", "FED.TRIM_K", 1]))
    with pytest.raises(ValueError, match="FED.ROBUST_AGG"):
        build_trainer(small_cfg(tmp_path / "bad2", clients=2, extra=["FED.ROBUST_AGG", "krum"]))


def test_robust_agg_none_is_the_parent(dev, tmp_path):
    off = build_trainer(small_cfg(tmp_path / "off", clients=2, extra=["FED.ROBUST_AGG", "none", "FED.TRIM_K", 2]))
    plain = build_trainer(small_cfg(tmp_path / "plain", clients=2))  # no mention of the new keys
    assert all(f.robust is None and f.trim is None and not f.weighted for f in off.fed + plain.fed)
    for c in off.clients:
        g = torch.Generator().manual_seed(3000 + c.client_id)
        e = c.engine
        e.flat16.add_((2.0 ** -6 * torch.randn(e.n16, generator=g)).half().to(dev))
        e.flat32.add_((2.0 ** -6 * torch.randn(e.n32, generator=g)).to(dev))
    snaps = [_snap(c) for c in off.clients]
    for a, b in zip(off.clients, plain.clients):
        b.engine.flat16.copy_(a.engine.flat16)
        b.engine.flat32.copy_(a.engine.flat32)
    assert off._fedavg([]) == 2 and plain._fedavg([]) == 2
    for a, b in zip(off.clients, plain.clients):
        assert torch.equal(a.engine.flat16, b.engine.flat16) and torch.equal(a.engine.flat32, b.engine.flat32)
    for n in snaps[0]:  # ... which is the reference's mean, rounded to fp16
        want = ((snaps[0][n].float() + snaps[1][n].float()) / 2).half()
        assert torch.equal(off.clients[0].engine.P[n].detach().cpu().float(), want.float()), n
