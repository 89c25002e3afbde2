"""GPU tier: FedDyn (Acar et al., ICLR 2021) -- the dynamic SGD kernels (mf_sgd_dyn_step / mf_optimizer_step_dyn), the
round's end (mf_feddyn_step / mf_feddyn_deliver) and the option through the trainer (FED.DYN_ALPHA).

Host restatements: host_dyn_step here (the dynamic step op by op in fp32, every line rounded to the buffer's dtype, in
the style of host_prox_step, whose lines it shares) and host_round_end of tests/test_feddyn_dist.py, which that file
ties to the paper's Algorithm 1 and to hand-worked values."""
import pytest
import torch

from federated_multi_modal_amd import ops
from federated_multi_modal_amd.trainers import build_trainer

from test_feddyn_dist import Replay, host_round_end
from test_fedopt_dist import _f
from test_fedprox_weighted_gpu import CASES, KEYS, LR, MOM, SIZES, WD, _rt, _run, _State, small_cfg

pytestmark = pytest.mark.gpu

ALPHA = 0.5


# ----------------------------------------------------------------------------- the local step

def host_dyn_step(p, g, buf, q, lam, coef, lr, mom, wd, alpha, first):
    """The dynamic step op by op on the host (CPU tensors of dtype T in, lam fp32; (p, g, buf) of dtype T out):
    gc = T(g*coef); d = T(p - q); gp = T(gc + alpha*d); gl = T(gp - lam); dp = T(gl + wd*p);
    b = dp | T(T(buf*mom) + dp); p = T(p - lr*b).  Scalars in fp32; every product, sum and difference is one fp32
    torch op (no fused multiply-add)."""
    T = p.dtype
    f = lambda v: torch.as_tensor(v, dtype=torch.float32)  # noqa: E731
    pf = p.float()
    gc = _rt(g.float() * f(coef), T)
    d = _rt(pf - q.float(), T)
    gp = _rt(gc + f(alpha) * d, T)
    gl = _rt(gp - lam, T)
    dp = _rt(gl + f(wd) * pf, T)
    b = dp if first else _rt(_rt(buf.float() * f(mom), T) + dp, T)
    pn = _rt(pf + f(-lr) * b, T)
    return pn.to(T), gc.to(T), b.to(T)


def _lam(st, zero=False):
    n = st.n16 + st.n32
    if zero:
        return torch.zeros(n)
    return 0.05 * torch.randn(n, generator=torch.Generator().manual_seed(77))


def _run_dyn(st, dev, api, alpha, lam, steps=1, halt=0.0, same_global=False):
    """_run of the proximal tests with the dynamic entry points: `lam` (host, n16 + n32 fp32) becomes one device array
    in the bucket's order, `off` elements into its allocation as every other buffer of the case."""
    d = st.device(dev, same_global)
    d["lam"] = st._dev(lam, dev)
    chunks, nchunks = st.chunks(dev)
    part = torch.empty(nchunks, device=dev)
    out = torch.empty(3, device=dev)
    hyper = torch.tensor([LR, MOM, WD, 1.0, halt, alpha], device=dev)
    halt_src = torch.zeros(1, device=dev)
    coefs = []
    for s in range(steps):
        if s:
            d["g16"].copy_(st.grads[s][0])
            d["g32"].copy_(st.grads[s][1])
            hyper[3] = 0.0
        if api == "fused":
            ops.optimizer_step_dyn(d["p16"], d["g16"], d["b16"], d["p32"], d["g32"], d["b32"], chunks, nchunks, 1.0,
                                   part, out, hyper, halt_src, None, d["q16"], d["q32"], d["lam"])
        else:
            ops.clip_grad_norm(d["g16"], d["g32"], chunks, nchunks, 1.0, part, out)
            ops.sgd_dyn_step(d["p16"], d["g16"], d["b16"], d["q16"], d["lam"][:st.n16], out, hyper)
            ops.sgd_dyn_step(d["p32"], d["g32"], d["b32"], d["q32"], d["lam"][st.n16:], out, hyper)
        coefs.append(out[1].item())
    torch.cuda.synchronize()
    return d, coefs


@pytest.fixture(scope="module")
def states():
    return {c: _State(c) for c in SIZES}


@pytest.mark.parametrize("case,api", CASES)
def test_dyn_zero_lam_is_the_proximal_step_bit_for_bit(dev, states, case, api):
    """GPU against GPU, two steps (first-step and momentum paths), mu = alpha."""
    st = states[case]
    a, _ = _run_dyn(st, dev, api, ALPHA, _lam(st, zero=True), steps=2)
    b, _ = _run(st, dev, api, ALPHA, prox=True, steps=2)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["p16"].cpu(), st.p16)  # a step was taken


@pytest.mark.parametrize("case,api", CASES)
def test_dyn_zero_lam_at_the_global_weights_is_the_plain_step(dev, states, case, api):
    st = states[case]
    a, _ = _run_dyn(st, dev, api, ALPHA, _lam(st, zero=True), same_global=True)
    b, _ = _run(st, dev, api, 0.0, prox=False, same_global=True)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case,api", CASES)
def test_dyn_step_equals_the_host_restatement(dev, states, case, api):
    """Two steps at alpha = 0.5, lam ~ 0.05 * randn, against host_dyn_step fed the device's own clip coefficient: IEEE
    fp32 operations in the same order with the same roundings on both sides, so bit for bit -- p, the stored (clipped)
    gradient and the momentum, fp16 and fp32.  lam is read only."""
    st = states[case]
    lam = _lam(st)
    d, coefs = _run_dyn(st, dev, api, ALPHA, lam, steps=2)
    d0, _ = _run_dyn(st, dev, api, ALPHA, _lam(st, zero=True), steps=2)
    h = {"p16": st.p16, "p32": st.p32, "b16": torch.zeros_like(st.p16), "b32": torch.zeros_like(st.p32)}
    for s in range(2):
        for k, q, lm in (("16", st.q16, lam[:st.n16]), ("32", st.q32, lam[st.n16:])):
            h["p" + k], h["g" + k], h["b" + k] = host_dyn_step(h["p" + k], st.grads[s][k == "32"], h["b" + k], q, lm,
                                                               coefs[s], LR, MOM, WD, ALPHA, s == 0)
    # the test can fail: the linear term changes most of the momentum buffer
    assert (d["b16"] != d0["b16"]).float().mean().item() > 0.5
    assert (d["b32"] != d0["b32"]).float().mean().item() > 0.5
    for k in KEYS:
        assert torch.equal(d[k].cpu(), h[k]), k
    assert torch.equal(d["lam"].cpu(), lam)


@pytest.mark.parametrize("case,api", CASES)
def test_dyn_halt_leaves_everything_untouched(dev, states, case, api):
    st = states[case]
    lam = _lam(st)
    d, _ = _run_dyn(st, dev, api, ALPHA, lam, halt=1.0)
    assert torch.equal(d["p16"].cpu(), st.p16) and torch.equal(d["p32"].cpu(), st.p32)
    assert torch.equal(d["g16"].cpu(), st.grads[0][0]) and torch.equal(d["g32"].cpu(), st.grads[0][1])
    assert not d["b16"].any() and not d["b32"].any()
    assert torch.equal(d["lam"].cpu(), lam)


def test_dyn_argument_validation(dev):
    n = 64
    p, g, b, q = (torch.zeros(n, dtype=torch.float16, device=dev) for _ in range(4))
    lam = torch.zeros(n, device=dev)
    out = torch.ones(3, device=dev)
    hyper5 = torch.tensor([LR, MOM, WD, 1.0, 0.0], device=dev)
    hyper6 = torch.tensor([LR, MOM, WD, 1.0, 0.0, 0.5], device=dev)
    with pytest.raises(ValueError):
        ops.sgd_dyn_step(p, g, b, q, lam, out, hyper5)         # alpha lives at hyper[5]
    with pytest.raises(ValueError):
        ops.sgd_dyn_step(p, g, b, q, lam.half(), out, hyper6)  # lam is fp32 whatever the buffer
    with pytest.raises(ValueError):
        ops.sgd_dyn_step(p, g, b, q, lam[:32], out, hyper6)
    with pytest.raises(ValueError):
        ops.sgd_dyn_step(p, g, b, q, lam.cpu(), out, hyper6)
    with pytest.raises(ValueError):
        ops.sgd_dyn_step(p, g, b, q, torch.zeros(2 * n, device=dev)[::2], out, hyper6)
    with pytest.raises(ValueError):
        ops.sgd_dyn_step(p, g, b, p, lam, out, hyper6)         # the global copy is a buffer of its own
    p32, g32, b32, q32 = (torch.zeros(n, device=dev) for _ in range(4))
    with pytest.raises(ValueError):
        ops.sgd_dyn_step(p32, g32, b32, q32, g32, out, hyper6)  # ... and so is lam
    ops.sgd_dyn_step(p, g, b, q, lam, out, hyper6)
    st = _State("vector")
    chunks, nchunks = st.chunks(dev)
    d = st.device(dev)
    part = torch.empty(nchunks, device=dev)
    halt_src = torch.zeros(1, device=dev)
    args = (d["p16"], d["g16"], d["b16"], d["p32"], d["g32"], d["b32"], chunks, nchunks, 1.0, part, out)
    full = torch.zeros(st.n16 + st.n32, device=dev)
    with pytest.raises(ValueError):
        ops.optimizer_step_dyn(*args, hyper6, halt_src, None, d["q16"], d["q32"])            # no lam
    with pytest.raises(ValueError):
        ops.optimizer_step_dyn(*args, hyper6, halt_src, None, d["q16"], d["q32"], full[:-1])
    with pytest.raises(ValueError):
        ops.optimizer_step_dyn(*args, hyper5, halt_src, None, d["q16"], d["q32"], full)
    with pytest.raises(ValueError):
        ops.optimizer_step_dyn(*args, hyper6, halt_src, None, d["p16"], d["q32"], full)
    with pytest.raises(ValueError):
        ops.optimizer_step_dyn(*args, hyper6, halt_src, None, d["q16"], d["q32"], d["q32"].new_zeros(st.n16 + st.n32,
                                                                                                   dtype=torch.float64))


# ----------------------------------------------------------------------------- the round's end

# (n16, n32): the scalar path with ragged tails; 8 per thread; 8 per thread with the fp16 / fp32 boundary in the last
# blocks (fp16: two full blocks of 256 threads and three threads of a third, fp32: five threads); the scalar path with
# the boundary in its last block; either buffer empty on either path
SHAPES = [(37, 4099), (4096, 2048), (4120, 40), (4099, 37), (0, 520), (520, 0), (0, 37), (37, 0)]


def _client(c, rnd, g16, g32):
    """A client's local result from the global weights, spread over binades as _client of the proximal tests spreads
    its values: relative steps of 2^-3, 2^-8 or 1 per round, as tests/test_fedopt_dist.py's local_result."""
    g = torch.Generator().manual_seed(9000 + 100 * rnd + c)
    scale = (2.0 ** -3, 2.0 ** -8, 1.0)[rnd % 3]
    p16 = (g16.float() + scale * 0.5 * torch.randn(g16.numel(), generator=g)).half()
    p32 = g32 + scale * (torch.randn(g32.numel(), generator=g) * g32.abs()
                         + 1e-3 * torch.randn(g32.numel(), generator=g))
    return p16, p32


class _DevGroup:
    """Three clients of one process on the device: each its weights, global copy, lam and flag; one h.  round() packs,
    sums in client order, runs mf_feddyn_step for client 0 and mf_feddyn_deliver for the others."""

    def __init__(self, dev, n16, n32, num_clients, alpha, clients=3):
        rp = Replay(num_clients, alpha, n16, n32)
        self.dev, self.n16, self.n32, self.N, self.alpha, self.C = dev, n16, n32, num_clients, alpha, clients
        n = n16 + n32
        self.g = [(rp.g16.to(dev), rp.g32.to(dev)) for _ in range(clients)]
        self.p = [(a.clone(), b.clone()) for a, b in self.g]
        self.lam = [torch.zeros(n, device=dev) for _ in range(clients)]
        self.flag = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(clients)]
        self.h = torch.zeros(n, device=dev)
        self.gathered = torch.empty(clients, n + 1, device=dev)
        self.total = torch.empty(n + 1, device=dev)

    def round(self, results, invalid=()):
        for c in range(self.C):
            self.p[c][0].copy_(results[c][0])
            self.p[c][1].copy_(results[c][1])
            self.flag[c].fill_(int(c in invalid))
            ops.fedavg_pack(self.p[c][0], self.p[c][1], self.flag[c], self.gathered[c])
        ops.fedavg_reduce_ordered(self.gathered.view(-1), self.C, self.total)
        for c in range(self.C):
            if c == 0:
                ops.feddyn_step(self.total, self.alpha, self.N, self.h, self.lam[c], self.flag[c], *self.p[c],
                                *self.g[c])
            else:
                ops.feddyn_deliver(self.total, self.alpha, self.h, self.lam[c], self.flag[c], *self.p[c], *self.g[c])
        torch.cuda.synchronize()

    def check(self, rp, what):
        for c in range(self.C):
            for name, got, want in (("p16", self.p[c][0], rp.g16), ("p32", self.p[c][1], rp.g32),
                                    ("g16", self.g[c][0], rp.g16), ("g32", self.g[c][1], rp.g32),
                                    ("lam", self.lam[c], rp.lam[c])):
                assert torch.equal(got.cpu(), want), f"{what}: client {c} {name}"
        assert torch.equal(self.h.cpu(), rp.h), f"{what}: h"


@pytest.mark.parametrize("n16,n32", SHAPES)
@pytest.mark.parametrize("num_clients", [3, 4])
def test_round_end_equals_the_host_restatement(dev, n16, n32, num_clients):
    """Three local clients, N = 3 and N = 4 (frac = 3 / 4: a fourth client that never shows up), against the replay of
    host_round_end, bit for bit on p16, p32, g16, g32, h and every lam: two consecutive full rounds (client 0 through
    mf_feddyn_step, clients 1 and 2 through mf_feddyn_deliver), a round with client 1's flag set (it keeps its lam and
    the sum excludes it), one with client 0's (the step still runs, from the others' sum), and a round with no vote."""
    grp = _DevGroup(dev, n16, n32, num_clients, 0.1)
    rp = Replay(num_clients, 0.1, n16, n32)
    for rnd in range(2):
        results = {c: _client(c, rnd, rp.g16, rp.g32) for c in range(3)}
        grp.round(results)
        rp.round([0, 1, 2], rnd, results)
        grp.check(rp, f"round {rnd}")
    assert rp.h.any() and all(rp.lam[c].any() for c in range(3))
    assert not torch.equal(rp.lam[1], rp.lam[2])  # each delivered client updated its own
    for rnd, out in ((2, 1), (3, 0)):
        results = {c: _client(c, rnd, rp.g16, rp.g32) for c in range(3)}
        kept = grp.lam[out].clone()
        grp.round(results, invalid=(out,))
        rp.round([c for c in range(3) if c != out], rnd, results)
        grp.check(rp, f"round {rnd}")
        assert torch.equal(grp.lam[out], kept)
    # no vote: every client goes back to its global copy; h and every lam keep their bits
    results = {c: _client(c, 4, rp.g16, rp.g32) for c in range(3)}
    grp.round(results, invalid=(0, 1, 2))
    assert grp.total[n16 + n32].item() == 0.0
    grp.check(rp, "the round without a vote")


def test_round_end_argument_validation(dev):
    n16, n32 = 16, 8
    n = n16 + n32
    p16, g16 = (torch.zeros(n16, dtype=torch.float16, device=dev) for _ in range(2))
    p32, g32 = (torch.zeros(n32, device=dev) for _ in range(2))
    h, lam = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    bucket = torch.ones(n + 1, device=dev)
    ops.feddyn_step(bucket, 0.1, 2, h, lam, flag, p16, p32, g16, g32)
    ops.feddyn_deliver(bucket, 0.1, h, lam, flag, p16, p32, g16, g32)
    for alpha in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.feddyn_step(bucket, alpha, 2, h, lam, flag, p16, p32, g16, g32)
        with pytest.raises(ValueError):
            ops.feddyn_deliver(bucket, alpha, h, lam, flag, p16, p32, g16, g32)
    for nc in (0, -1, 1.5):
        with pytest.raises(ValueError):
            ops.feddyn_step(bucket, 0.1, nc, h, lam, flag, p16, p32, g16, g32)
    for kw in (dict(bucket=bucket[:n]), dict(h=h[:-1]), dict(lam=lam.double()), dict(lam=h), dict(h=bucket[:n]),
               dict(flag=flag.float()), dict(g16=p16), dict(p32=p32.half()), dict(lam=lam.cpu())):
        a = dict(bucket=bucket, h=h, lam=lam, flag=flag, p16=p16, p32=p32, g16=g16, g32=g32)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.feddyn_step(a["bucket"], 0.1, 2, a["h"], a["lam"], a["flag"], a["p16"], a["p32"], a["g16"], a["g32"])
        with pytest.raises(ValueError):
            ops.feddyn_deliver(a["bucket"], 0.1, a["h"], a["lam"], a["flag"], a["p16"], a["p32"], a["g16"], a["g32"])
    # the C entry points check for themselves
    from federated_multi_modal_amd._lib import MapfedError, call
    with pytest.raises(MapfedError, match="alpha"):
        call("mf_feddyn_step", bucket.data_ptr(), 0.0, 2, h.data_ptr(), lam.data_ptr(), flag.data_ptr(),
             p16.data_ptr(), n16, p32.data_ptr(), n32, g16.data_ptr(), g32.data_ptr(), None)
    with pytest.raises(MapfedError, match="num_clients"):
        call("mf_feddyn_step", bucket.data_ptr(), 0.1, 0, h.data_ptr(), lam.data_ptr(), flag.data_ptr(),
             p16.data_ptr(), n16, p32.data_ptr(), n32, g16.data_ptr(), g32.data_ptr(), None)
    with pytest.raises(MapfedError, match="negative"):
        call("mf_feddyn_deliver", bucket.data_ptr(), 0.1, h.data_ptr(), lam.data_ptr(), flag.data_ptr(),
             p16.data_ptr(), -1, p32.data_ptr(), n32, g16.data_ptr(), g32.data_ptr(), None)
    with pytest.raises(MapfedError, match="null"):
        call("mf_feddyn_deliver", bucket.data_ptr(), 0.1, None, lam.data_ptr(), flag.data_ptr(),
             p16.data_ptr(), n16, p32.data_ptr(), n32, g16.data_ptr(), g32.data_ptr(), None)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- through the trainer

def test_dynamic_trainer_beside_a_plain_one(dev, tmp_path):
    # the config's warm-up learning rate (1e-4) moves hardly any fp16 weight in one step; 0.01 moves many
    lr = ["OPTIM.WARMUP_CONS_LR", 0.01]
    dyn = build_trainer(small_cfg(tmp_path / "dyn", extra=["FED.DYN_ALPHA", 0.1] + lr))
    plain = build_trainer(small_cfg(tmp_path / "plain", extra=lr))
    alpha = float(_f(0.1))
    state = dyn.dyn
    assert state is not None and state.alpha == 0.1 and state.num_clients == 2 and getattr(plain, "dyn", None) is None
    ca, cb = dyn.clients[0], plain.clients[0]
    ea, eb = ca.engine, cb.engine
    n16 = ea.n16
    assert eb._prox["glob"] is None and eb._prox["lam"] is None

    def holds_the_buckets_buffers():
        for c, fed in zip(dyn.clients, dyn.fed):
            assert c.engine._prox["lam"] is fed.lam
            assert c.engine._prox["glob"][0] is fed.global16 and c.engine._prox["glob"][1] is fed.global32

    holds_the_buckets_buffers()
    assert ea.hyper[5].item() == alpha and not state.h.any() and not dyn.fed[0].lam.any()
    batch = next(iter(cb.dm.train_loader))
    # step 1 (eager, first_step): lam = 0 and the weights equal the global copy, so both terms are exactly zero
    ca.forward_backward(batch)
    cb.forward_backward(batch)
    for k in ("flat16", "flat32", "mom16", "mom32", "gflat16", "gflat32"):
        assert torch.equal(getattr(ea, k), getattr(eb, k)), k
    assert not torch.equal(ea.flat32, dyn.fed[0].global32)
    c1 = dyn.clients[1]
    c1.forward_backward(next(iter(c1.dm.train_loader)))
    # the round's end against the restatement, from the local weights saved before it
    ws = [torch.cat([c.engine.flat16.float(), c.engine.flat32]).cpu() for c in dyn.clients]
    q = torch.cat([dyn.fed[0].global16.float(), dyn.fed[0].global32]).cpu()
    assert dyn._fedavg([]) == 2
    total, votes = ws[0] + ws[1], _f(2.0)
    x, h, lam0 = host_round_end(total, votes, 2, 0.1, ws[0], q, torch.zeros_like(q), torch.zeros_like(q), True, True)
    _, _, lam1 = host_round_end(total, votes, 2, 0.1, ws[1], q, h, torch.zeros_like(q), True, False)
    assert torch.equal(dyn.fed[0].lam.cpu(), lam0) and torch.equal(dyn.fed[1].lam.cpu(), lam1)
    assert torch.equal(state.h.cpu(), h) and lam0.any() and lam1.any() and h.any()
    val = x.half()
    for c, fed in zip(dyn.clients, dyn.fed):  # every client sits at the global copy
        assert torch.equal(fed.global16, c.engine.flat16) and torch.equal(fed.global32, c.engine.flat32)
        assert torch.equal(fed.global16.cpu(), val[:n16]) and torch.equal(fed.global32.cpu(), val[n16:].float())
    holds_the_buckets_buffers()
    # the next step (the captured graph, first step after the broadcast) beside a plain step from the same weights:
    # the weights equal the global copy, so what differs is lam, read by the captured step
    eb.flat16.copy_(ea.flat16)
    eb.flat32.copy_(ea.flat32)
    eb.after_weights_loaded()
    p32_before = ea.flat32.clone()
    ca.forward_backward(batch)
    cb.forward_backward(batch)
    assert ca._graphs and ea._prox["captured"]
    assert not torch.equal(ea.flat32, eb.flat32) and not torch.equal(ea.mom32, eb.mom32)
    assert not torch.equal(ea.mom16, eb.mom16)
    lr_, mom, wd, first, halt, a = ea.hyper.tolist()
    assert halt == 0.0 and a == alpha
    _, _, want32 = host_dyn_step(p32_before.cpu(), ea.gflat32.cpu(), torch.zeros_like(q[n16:]),
                                 dyn.fed[0].global32.cpu(), lam0[n16:], 1.0, lr_, mom, wd, a, True)
    torch.testing.assert_close(ea.mom32.cpu(), want32, rtol=1e-6, atol=1e-7)
    with pytest.raises(RuntimeError):
        ea.set_dynamic(0.1, dyn.fed[0].global16, dyn.fed[0].global32, dyn.fed[0].lam)  # a step is captured


def test_full_round_with_dyn_alpha(dev, tmp_path):
    tr = build_trainer(small_cfg(tmp_path, extra=["FED.DYN_ALPHA", 0.1]))
    tr.train()
    assert tr.nan_stats["total_updates"] == 1 and tr.nan_stats["skipped_rounds"] == 0
    for c, fed in zip(tr.clients, tr.fed):
        assert torch.equal(fed.global16, c.engine.flat16) and torch.equal(fed.global32, c.engine.flat32)
        assert c.engine._prox["lam"] is fed.lam and fed.lam.any()
    assert tr.dyn.h.any() and not tr.dyn.pending


def test_dyn_alpha_zero_builds_nothing_and_the_rejected_combinations(dev, tmp_path):
    tr = build_trainer(small_cfg(tmp_path / "off", extra=["FED.DYN_ALPHA", 0.0]))
    assert tr.dyn is None and all(fed.dyn is None and fed.lam is None for fed in tr.fed)
    e = tr.clients[0].engine
    assert e._prox["glob"] is None and e._prox["lam"] is None and e.hyper[5].item() == 0.0  # the plain launch
    # mu and alpha share hyper[5]: the one that is in effect refuses the other (no step is captured yet)
    fed, lam = tr.fed[0], torch.zeros(e.n16 + e.n32, device=dev)
    e.set_proximal(0.5, fed.global16, fed.global32)
    with pytest.raises(ValueError):
        e.set_dynamic(0.1, fed.global16, fed.global32, lam)
    e1, fed1 = tr.clients[1].engine, tr.fed[1]
    e1.set_dynamic(0.1, fed1.global16, fed1.global32, lam)
    assert e1._prox["lam"] is lam and e1.hyper[5].item() == float(torch.tensor(0.1))
    with pytest.raises(ValueError):
        e1.set_proximal(0.5, fed1.global16, fed1.global32)
    with pytest.raises(ValueError):
        e1.set_dynamic(0.1, fed1.global16, fed1.global32, lam[:-1])
    with pytest.raises(ValueError):
        e1.set_dynamic(0.0, fed1.global16, fed1.global32, lam)
    for i, (bad, key) in enumerate(((["FED.PROX_MU", 0.5], "PROX_MU"), (["FED.SERVER_OPT", "fedadam"], "SERVER_OPT"),
                                    (["FED.CLIENT_WEIGHTS", "3,1"], "CLIENT_WEIGHTS"),
                                    (["FED.ROBUST_AGG", "median"], "ROBUST_AGG"), (["FED.DP_CLIP", 1.0], "DP_CLIP"),
                                    (["FED.COMPRESS", "int8"], "COMPRESS"))):
        with pytest.raises(ValueError, match="FED." + key):
            build_trainer(small_cfg(tmp_path / f"bad{i}", extra=["FED.DYN_ALPHA", 0.1] + bad))
    with pytest.raises(ValueError, match="FED.DYN_ALPHA"):
        build_trainer(small_cfg(tmp_path / "neg", extra=["FED.DYN_ALPHA", -0.1]))
