"""GPU tier: the FedOpt server-step kernels (mf_fedopt_step / mf_fedopt_deliver: FedAvgM, Hsu et al. 2019; FedAdagrad /
FedAdam / FedYogi, Reddi et al., ICLR 2021) against the host restatement of tests/test_fedopt_dist.py (host_step:
torch fp32 on the CPU, one op per rounding point) bit for bit, the step over the RCCL chain, and FED.SERVER_OPT
through the trainer.

Bit for bit means: the kernel's fp32 operations are IEEE (correctly rounded division and square root, no fused
multiply-add, round to nearest even), in the restatement's order.  That holds for normal numbers and exact zeros,
which is all the inputs below produce (see _case); denormal behaviour is not pinned by these tests."""
import socket

import pytest
import torch
import torch.distributed as dist

from federated_multi_modal_amd import _lib, ops
from federated_multi_modal_amd.federated import FedAvgBucket, ServerOptimizer
from federated_multi_modal_amd.trainers import build_trainer
from test_fedopt_dist import HP, NAMES, OPTS, FedOptHostKernels, _f, host_step
from test_fedprox_weighted_gpu import small_cfg

pytestmark = pytest.mark.gpu

# (n16, n32): the scalar path with ragged tails (the shape of test_fedprox_weighted_gpu._client); the 8-wide path; the
# fp16 / fp32 boundary inside the launch's last blocks (3 fp16 blocks, the third one ninth full, then 1 fp32 block of
# one thread); either buffer empty
SHAPES = [(37, 4096 + 3), (4096, 1024), (4096 + 8, 8), (4096, 0), (0, 1024)]


def _case(opt, n16, n32, weighted, seed=0):
    """Host inputs of two rounds.  State x spread over twelve binades (2^-6 .. 2^5 times a normal deviate), buckets
    whose mean lies |Delta| in [2^-14, 4] away from x (up to the rounding of the mean), every
    eighth element at Delta = 0 exactly in round one; for the adaptive optimizers v starts at tau^2 except where it
    is set on either side of s = Delta^2 and exactly at it (FedYogi's three branches; harmless for the other two).
    Magnitudes: every non-zero operand is at least 2^-36 (the smallest, (1 - beta2) * s with s >= 2^-28), so a
    non-zero sum or difference is at least 2^-60 and no intermediate is denormal."""
    g = torch.Generator().manual_seed(1234 + seed)
    n = n16 + n32
    d = _f(4.0) if weighted else _f(3.0)  # weights (2, 1, 1) / three votes
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 6, (n,), generator=g).float())
    x = torch.where(x.abs() < 2.0 ** -8, torch.full_like(x, 0.5), x)
    x[:n16] = x[:n16].half().float()

    def bucket_for(xcur, with_zeros):
        mag = torch.exp2(torch.rand(n, generator=g) * 16.0 - 14.0)        # 2^-14 .. 4
        delta = mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        total = (xcur + delta) * d
        if with_zeros:
            zero = torch.arange(n) % 8 == 2
            if weighted:  # d = 4: x * 4 / 4 is x
                total = torch.where(zero, xcur * d, total)
        tail = [float(d), 3.0] if weighted else [3.0]
        return torch.cat([total, torch.tensor(tail)])

    b1 = bucket_for(x, True)
    if not weighted:
        # d = 3: the elements with Delta = 0 take their x from the bucket, x = fp32(total / 3)
        zero = torch.arange(n) % 8 == 2
        x = torch.where(zero, b1[:n] / d, x)
    m = torch.zeros(n)
    v = None
    if opt != "fedavgm":
        tau2 = float(_f(HP["tau"]) * _f(HP["tau"]))
        v = torch.full((n,), tau2)
        delta = b1[:n] / d - x
        s = delta * delta  # the kernel's s of round one, formed the same way
        idx = torch.arange(n)
        v = torch.where((idx % 8 == 3) & (s > 0), s, v)            # v == s
        v = torch.where((idx % 8 == 4) & (s > 0), 4.0 * s, v)      # v > s
        v = torch.where((idx % 8 == 5) & (s > 0), 0.25 * s, v)     # v < s
        if opt == "fedyogi":
            side = torch.sign(v - s)
            assert (side == 0).any() and (side > 0).any() and (side < 0).any()
    assert ((b1[:n] / d - x) == 0).sum().item() >= n // 8
    return {"x": x, "m": m, "v": v, "b1": b1, "bucket_for": bucket_for, "d": d}


def _host_round(opt, bucket, weighted, st, n16):
    """The restatement on CPU tensors, in place (FedOptHostKernels.fedopt_step, what the gloo tests run)."""
    FedOptHostKernels.fedopt_step(bucket, weighted, opt, HP["beta1"], HP["beta2"], HP["tau"], HP["lr"], st["x"], st["m"],
                                  st["v"], st["p16"], st["p32"], st["g16"], st["g32"])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n16,n32", SHAPES)
@pytest.mark.parametrize("opt", OPTS)
def test_step_kernel_equals_the_host_restatement(dev, opt, n16, n32, weighted):
    c = _case(opt, n16, n32, weighted)
    host = {"x": c["x"].clone(), "m": c["m"].clone(), "v": None if c["v"] is None else c["v"].clone(),
            "p16": torch.zeros(n16, dtype=torch.float16), "p32": torch.zeros(n32),
            "g16": c["x"][:n16].half(), "g32": c["x"][n16:].half().float()}
    d = {k: (None if t is None else t.to(dev)) for k, t in host.items()}
    x_start = host["x"].clone()
    for rnd in range(2):
        bucket = c["b1"] if rnd == 0 else c["bucket_for"](host["x"], False)
        _host_round(opt, bucket, weighted, host, n16)
        ops.fedopt_step(bucket.to(dev), weighted, opt, HP["beta1"], HP["beta2"], HP["tau"], HP["lr"], d["x"], d["m"],
                        d["v"], d["p16"], d["p32"], d["g16"], d["g32"])
        torch.cuda.synchronize()
        for k in NAMES:
            if host[k] is None:
                assert d[k] is None
                continue
            same = torch.equal(d[k].cpu(), host[k])
            if not same:
                bad = (d[k].cpu() != host[k]).nonzero().flatten()
                print(f"{opt} round {rnd} {k}: {bad.numel()} of {host[k].numel()} differ, first at {bad[:5].tolist()}")
            assert same, (opt, rnd, k)
    assert not torch.equal(host["x"], x_start)  # steps were taken


@pytest.mark.parametrize("n16,n32", SHAPES[:2])
@pytest.mark.parametrize("opt", ["fedavgm", "fedyogi"])
def test_no_votes_reverts_and_keeps_the_state(dev, opt, n16, n32):
    c = _case(opt, n16, n32, True)
    bucket = c["b1"].clone()
    bucket[-1] = 0.0  # the vote count; the sum and the summed weights stay non-zero and must not be read as valid
    x, m = c["x"].to(dev), torch.full_like(c["x"], 0.25).to(dev)
    v = None if c["v"] is None else c["v"].to(dev)
    g16 = torch.full((n16,), 3.0, dtype=torch.float16, device=dev)
    g32 = torch.full((n32,), 5.0, device=dev)
    p16, p32 = torch.zeros_like(g16), torch.zeros_like(g32)
    ops.fedopt_step(bucket.to(dev), True, opt, HP["beta1"], HP["beta2"], HP["tau"], HP["lr"], x, m, v, p16, p32, g16, g32)
    torch.cuda.synchronize()
    assert torch.equal(p16, g16) and torch.equal(p32, g32)
    assert (g16 == 3.0).all() and (g32 == 5.0).all()
    assert torch.equal(x.cpu(), c["x"]) and (m == 0.25).all()
    assert v is None or torch.equal(v.cpu(), c["v"])


@pytest.mark.parametrize("n16,n32", SHAPES)
def test_deliver_writes_the_bits_of_the_step(dev, n16, n32):
    c = _case("fedadam", n16, n32, False)
    x, m, v = c["x"].to(dev), c["m"].to(dev), c["v"].to(dev)
    mk = lambda: (torch.zeros(n16, dtype=torch.float16, device=dev), torch.zeros(n32, device=dev),  # noqa: E731
                  torch.zeros(n16, dtype=torch.float16, device=dev), torch.zeros(n32, device=dev))
    first, second = mk(), mk()
    ops.fedopt_step(c["b1"].to(dev), False, "fedadam", HP["beta1"], HP["beta2"], HP["tau"], HP["lr"], x, m, v, *first)
    state = (x.clone(), m.clone(), v.clone())
    ops.fedopt_deliver(x, *second)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert torch.equal(second[0].float(), x[:n16].half().float()) and torch.equal(second[1], x[n16:].half().float())
    assert torch.equal(second[0], second[2]) and torch.equal(second[1], second[3])
    assert all(torch.equal(a, b) for a, b in zip(state, (x, m, v)))


def test_argument_validation(dev):
    """Through ops every rejected call raises and a following good call succeeds; the launchers' own checks, reached
    through the C ABI, return an error and launch nothing."""
    n16, n32 = 64, 32
    n = n16 + n32
    mk = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    bucket = torch.ones(n + 2, device=dev)
    x, m, v = mk(n), mk(n), torch.ones(n, device=dev)
    p16, p32, g16, g32 = mk(n16, torch.float16), mk(n32), mk(n16, torch.float16), mk(n32)
    hp = (HP["beta1"], HP["beta2"], HP["tau"], HP["lr"])

    def good():
        ops.fedopt_step(bucket, True, "fedadam", *hp, x, m, v, p16, p32, g16, g32)
        ops.fedopt_step(bucket, False, "fedavgm", *hp, x, m, None, p16, p32, g16, g32)
        ops.fedopt_deliver(x, p16, p32, g16, g32)

    good()
    bad_calls = [
        lambda: ops.fedopt_step(bucket, True, "fedsgd", *hp, x, m, v, p16, p32, g16, g32),             # unknown optimizer
        lambda: ops.fedopt_step(bucket, True, "fedadam", 0.9, 0.99, 0.0, 0.1, x, m, v, p16, p32, g16, g32),   # tau <= 0
        lambda: ops.fedopt_step(bucket, True, "fedyogi", 0.9, 0.99, 1e-3, float("nan"), x, m, v, p16, p32, g16, g32),
        lambda: ops.fedopt_step(bucket, True, "fedavgm", float("inf"), 0.99, 1e-3, 0.1, x, m, None, p16, p32, g16, g32),
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x, m, None, p16, p32, g16, g32),         # no v
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, None, m, v, p16, p32, g16, g32),         # no x
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x.half(), m, v, p16, p32, g16, g32),     # dtype
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x, m[:n - 1], v, p16, p32, g16, g32),    # size
        lambda: ops.fedopt_step(bucket[:n + 1], True, "fedadam", *hp, x, m, v, p16, p32, g16, g32),    # bucket too short
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x, x, v, p16, p32, g16, g32),            # m is x
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x, m, m, p16, p32, g16, g32),            # v is m
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, bucket[:n], m, v, p16, p32, g16, g32),   # x in the bucket
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x, m, v, p16, p32, p16, g32),            # g16 is p16
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x, m, v, p16, x[n16:], g16, g32),        # p32 inside x
        lambda: ops.fedopt_step(bucket, True, "fedadam", *hp, x, m, v, p16.float(), p32, g16, g32),
        lambda: ops.fedopt_deliver(None, p16, p32, g16, g32),
        lambda: ops.fedopt_deliver(x[:n - 1], p16, p32, g16, g32),
        lambda: ops.fedopt_deliver(x, p16, x[n16:], g16, g32),
        lambda: ops.fedopt_deliver(x, p16, p32, g16[:8], g32),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
        good()
    # the C ABI's own checks
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    raw = lambda **kw: _lib.call("mf_fedopt_step", P(bucket), 1, kw.get("opt", 3), kw.get("b1", 0.9), 0.99,  # noqa: E731
                                 kw.get("tau", 1e-3), kw.get("eta", 0.1), P(kw.get("x", x)), P(m), P(kw.get("v", v)),
                                 P(p16), kw.get("n16", n16), P(p32), n32, P(g16), P(g32), None)
    for kw in (dict(n16=-1), dict(opt=0), dict(opt=5), dict(tau=0.0), dict(tau=-1.0), dict(eta=float("inf")),
               dict(b1=float("nan")), dict(x=None), dict(v=None)):
        with pytest.raises(_lib.MapfedError):
            raw(**kw)
    raw(opt=1, v=None, tau=0.0)  # fedavgm has no v and reads no tau
    with pytest.raises(_lib.MapfedError):
        _lib.call("mf_fedopt_deliver", None, P(p16), n16, P(p32), n32, P(g16), P(g32), None)
    with pytest.raises(_lib.MapfedError):
        _lib.call("mf_fedopt_deliver", P(x), P(p16), n16, P(p32), -2, P(g16), P(g32), None)
    good()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the RCCL chain at world size 1

class _Eng:
    def __init__(self, dev, n16, n32, seed):
        g = torch.Generator().manual_seed(seed)
        self.device = dev
        self.n16, self.n32 = n16, n32
        self.flat16 = (torch.randn(n16, generator=g) * 3).half().to(dev)
        self.flat32 = (torch.randn(n32, generator=g) * 1e-3).to(dev)
        self.loaded = 0

    def after_weights_loaded(self):
        self.loaded += 1


@pytest.fixture
def rccl_group(dev):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    yield
    dist.destroy_process_group()


def test_server_step_over_the_rccl_chain(dev, rccl_group):
    """all_to_all -> mf_fedavg_reduce_ordered -> all_gather on the side stream (shard_single), then one server step:
    with one client the sum is its weights and d = 1."""
    e = _Eng(dev, 100_003, 7_777, 3)
    server = ServerOptimizer("fedadam", e, **HP)
    fed = FedAvgBucket(e, mode="ordered", shard_single=True, server=server)
    assert fed.sharded and fed.side is not None
    x0 = torch.cat([e.flat16.float(), e.flat32]).cpu()
    g = torch.Generator().manual_seed(4)
    e.flat16.add_((0.05 * torch.randn(e.n16, generator=g)).half().to(dev))
    e.flat32.add_((1e-4 * torch.randn(e.n32, generator=g)).to(dev))
    local = torch.cat([e.flat16.float(), e.flat32]).cpu()
    fed.start()
    fed.finish()
    torch.cuda.synchronize()
    tau2 = float(_f(HP["tau"]) * _f(HP["tau"]))
    x, m, v = host_step("fedadam", local, _f(1.0), x0, torch.zeros_like(x0), torch.full_like(x0, tau2), **HP)
    assert fed.n_valid() == 1 and e.loaded == 1
    assert torch.equal(server.x.cpu(), x) and torch.equal(server.m.cpu(), m) and torch.equal(server.v.cpu(), v)
    val = x.half()
    assert torch.equal(e.flat16.cpu(), val[:e.n16]) and torch.equal(e.flat32.cpu(), val[e.n16:].float())
    assert torch.equal(fed.global16, e.flat16) and torch.equal(fed.global32, e.flat32)
    assert not torch.equal(x, x0)


# ----------------------------------------------------------------------------- through the trainer

# eta = 1 with an adaptive optimizer moves every weight by about one per round; 1e-3 keeps the model trainable
ADAM = ["FED.SERVER_OPT", "fedadam", "FED.SERVER_LR", 1e-3]
ADAM_HP = {"lr": 1e-3, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}


def _snap(c):
    return {n: c.engine.P[n].detach().clone().cpu() for n in c.engine.trainable_names}


class _TensorReplay:
    """The restatement tensor by tensor: x = float(initial weights), m = 0, v = tau^2, then one host_step per round
    on the clients' snapshots summed in client order."""

    def __init__(self, snap0, opt, hp):
        self.opt, self.hp = opt, hp
        tau2 = float(_f(hp["tau"]) * _f(hp["tau"]))
        self.x = {n: t.float() for n, t in snap0.items()}
        self.m = {n: torch.zeros_like(t) for n, t in self.x.items()}
        self.v = {n: (None if opt == "fedavgm" else torch.full_like(t, tau2)) for n, t in self.x.items()}

    def round(self, snaps):
        for n in self.x:
            acc = snaps[0][n].float()
            for s in snaps[1:]:
                acc = acc + s[n].float()
            self.x[n], self.m[n], self.v[n] = host_step(self.opt, acc, _f(len(snaps)), self.x[n], self.m[n], self.v[n],
                                                        **self.hp)

    def check(self, trainer):
        for c in trainer.clients:
            for n in self.x:
                assert torch.equal(c.engine.P[n].detach().cpu().float(), self.x[n].half().float()), n


def _copy_weights(src, dst):
    for a, b in zip(src.clients, dst.clients):
        b.engine.flat16.copy_(a.engine.flat16)
        b.engine.flat32.copy_(a.engine.flat32)


def _local_results(tr, seed):
    """Stand-ins for local training where the test is not about it: every client's weights moved off the global
    copy by a seeded perturbation of its own."""
    for c in tr.clients:
        g = torch.Generator().manual_seed(1000 * seed + c.client_id)
        e = c.engine
        e.flat16.add_((2.0 ** -6 * torch.randn(e.n16, generator=g)).half().to(e.flat16.device))
        e.flat32.add_((2.0 ** -6 * torch.randn(e.n32, generator=g)).to(e.flat32.device))


def _same_weights(a, b):
    return all(torch.equal(x.engine.flat16, y.engine.flat16) and torch.equal(x.engine.flat32, y.engine.flat32)
               for x, y in zip(a.clients, b.clients))


@pytest.fixture(scope="module")
def off_trainer(dev, tmp_path_factory):
    """A trainer with FED.SERVER_OPT none spelled out, and the checkpoint it writes."""
    out = tmp_path_factory.mktemp("off")
    tr = build_trainer(small_cfg(out, clients=2, extra=["FED.SERVER_OPT", "none", "FED.SERVER_LR", 0.5]))
    path = tr.save_model()
    return tr, out, path


def test_fedadam_two_rounds_through_the_trainer(dev, tmp_path):
    tr = build_trainer(small_cfg(tmp_path, clients=3, extra=ADAM))
    assert tr.server is not None and tr.server.name == "fedadam" and tr.server.hyper() == ADAM_HP
    assert all(f.server is tr.server for f in tr.fed)
    rp = _TensorReplay(_snap(tr.clients[0]), "fedadam", ADAM_HP)
    for rnd in range(2):  # the second round: the state carried over
        for c in tr.clients:
            c.run_epoch(rnd)
        snaps = [_snap(c) for c in tr.clients]
        assert not all(torch.equal(snaps[0][n], snaps[1][n]) for n in snaps[0])
        assert tr._fedavg([]) == 3
        rp.round(snaps)
        rp.check(tr)
    sv = tr.server
    assert sv.m.any() and torch.equal(sv.x[:sv.n16].half(), tr.fed[0].global16)


def test_checkpoint_carries_the_server_state(dev, tmp_path, off_trainer):
    tr = build_trainer(small_cfg(tmp_path / "a", clients=2, extra=ADAM))
    sv = tr.server
    _local_results(tr, 1)
    assert tr._fedavg([]) == 2 and sv.m.any()
    # save_model -> load_model into a fresh trainer: the state's bits, and the same next round
    path = tr.save_model()
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["server_optimizer"]["name"] == "fedadam" and ckpt["server_optimizer"]["hyper"] == ADAM_HP
    other = build_trainer(small_cfg(tmp_path / "b", clients=2, extra=ADAM))
    other.load_model(str(tmp_path / "a"), epoch=tr.cfg.OPTIM.MAX_EPOCH)
    assert _same_weights(tr, other)
    for k in ("x", "m", "v"):
        assert torch.equal(getattr(other.server, k), getattr(sv, k)), k
    _local_results(tr, 2)
    _copy_weights(tr, other)
    assert tr._fedavg([]) == 2 and other._fedavg([]) == 2
    assert _same_weights(tr, other)
    for k in ("x", "m", "v"):
        assert torch.equal(getattr(other.server, k), getattr(sv, k)), k
    # broadcast_weights with an explicit state dict restarts the server state from those weights
    other.broadcast_weights(ckpt["state_dict"])
    e0 = other.clients[0].engine
    assert torch.equal(other.server.x, torch.cat([e0.flat16.float(), e0.flat32])) and not other.server.m.any()
    assert torch.equal(other.fed[1].global16, other.clients[1].engine.flat16)
    # a checkpoint written with the feature off, loaded with it on: the state starts from the loaded weights
    off, off_dir, off_path = off_trainer
    assert torch.load(off_path, map_location="cpu", weights_only=True)["server_optimizer"] is None
    other.server.m.fill_(1.0)
    other.load_model(str(off_dir), epoch=off.cfg.OPTIM.MAX_EPOCH)
    saved = torch.load(off_path, map_location="cpu", weights_only=True)["state_dict"]
    now = other.clients[0].model.state_dict()
    assert all(torch.equal(now[k].detach().half().cpu(), saved[k]) for k in saved)
    tau2 = float(_f(1e-3) * _f(1e-3))
    assert torch.equal(other.server.x, torch.cat([e0.flat16.float(), e0.flat32]))
    assert not other.server.m.any() and (other.server.v == tau2).all()


def test_server_opt_none_is_the_parent(dev, tmp_path, off_trainer):
    off = off_trainer[0]
    plain = build_trainer(small_cfg(tmp_path / "plain", clients=2))  # no mention of the new keys
    assert off.server is None and plain.server is None and all(f.server is None for f in off.fed)
    _local_results(off, 3)
    snaps = [_snap(c) for c in off.clients]
    _copy_weights(off, plain)
    assert off._fedavg([]) == 2 and plain._fedavg([]) == 2
    assert _same_weights(off, plain)
    for n in snaps[0]:  # ... which is the reference's mean, rounded to fp16
        want = ((snaps[0][n].float() + snaps[1][n].float()) / 2).half()
        assert torch.equal(off.clients[0].engine.P[n].detach().cpu().float(), want.float()), n
    # config validation through build_trainer: the key is named (every bad value: tests/test_fedopt_dist.py)
    with pytest.raises(ValueError, match="FED.SERVER_TAU"):
        build_trainer(small_cfg(tmp_path / "bad", clients=2, extra=["FED.SERVER_OPT", "fedadam", "FED.SERVER_TAU", 0.0]))
    with pytest.raises(ValueError, match="FED.SERVER_OPT"):
        build_trainer(small_cfg(tmp_path / "bad2", clients=2, extra=["FED.SERVER_OPT", "fedsgd"]))


def test_fedavgm_with_client_weights_and_fedprox_through_train(dev, tmp_path):
    tr = build_trainer(small_cfg(tmp_path, clients=3, rounds=2, extra=[
        "FED.SERVER_OPT", "fedavgm", "FED.CLIENT_WEIGHTS", "3,1,2", "FED.PROX_MU", 0.5]))
    assert tr.server.v is None
    globs = [(f.global16.data_ptr(), f.global32.data_ptr()) for f in tr.fed]
    tr.train()
    assert tr.nan_stats["total_updates"] == 2 and tr.nan_stats["skipped_rounds"] == 0
    sv = tr.server
    for c, fed, ptrs in zip(tr.clients, tr.fed, globs):
        assert torch.equal(fed.global16, c.engine.flat16) and torch.equal(fed.global32, c.engine.flat32)
        assert torch.equal(fed.global16, tr.fed[0].global16) and torch.equal(fed.global32, tr.fed[0].global32)
        # refreshed in place: the captured proximal steps keep their pointers
        assert (fed.global16.data_ptr(), fed.global32.data_ptr()) == ptrs
        assert c.engine._prox["glob"][0] is fed.global16
    assert torch.equal(sv.x[:sv.n16].half(), tr.fed[0].global16)
    assert torch.equal(sv.x[sv.n16:].half().float(), tr.fed[0].global32) and sv.m.any()
