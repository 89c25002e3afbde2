"""GPU tier: the sample-weighted FedAvg kernels (mf_fedavg_pack_weighted / mf_fedavg_unpack_weighted; McMahan et
al., AISTATS 2017), the FedProx proximal SGD kernels (mf_sgd_prox_step / mf_optimizer_step_prox; Li et al., MLSys
2020) and both options through the trainer (FED.CLIENT_WEIGHTS, FED.PROX_MU).

Host restatements of the new arithmetic live here: weighted_reference (the torch CPU expression
acc = w0*x0; acc += wc*xc ...; (acc / sum w).half()) and host_prox_step (the proximal step op by op in fp32, every
line rounded to the buffer's dtype, the scalars in fp32 as the kernels read them from `hyper`)."""
import numpy as np
import pytest
import torch

from federated_multi_modal_amd import ops
from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
from federated_multi_modal_amd.trainers import build_trainer

pytestmark = pytest.mark.gpu

# lr = 0.1 and weight decay = 5e-4 at the nearest fp16 values (0.0999755859375, 0.0005002021789550781), handed to the
# kernels and to torch alike.  For Half tensors torch's CPU add(other, alpha=s) rounds the scalar s to fp16 before it
# multiplies (op by op on 100 000 elements: a restatement with alpha = fp16(s) equals torch on all but 1e-5 of them,
# one with alpha = fp32(s) differs on 2.5-9.5 % for s = 5e-4 and on 0.3-1 % for s = -0.1), so torch.optim.SGD on the
# CPU steps fp16 tensors with fp16(lr) and fp16(weight_decay) whatever it is given, while the kernels read fp32 scalars
# from `hyper`, as torch does on a GPU.  With values fp16 holds exactly both sides step with the same numbers; momentum
# (mul_, fp32 scalar on both sides) and mu = 0.5 need no such care.
LR = float(torch.tensor(0.1).half())
WD = float(torch.tensor(5e-4).half())
MOM = 0.9


# ----------------------------------------------------------------------------- weighted FedAvg kernels

def _client(seed, n16=37, n32=4096 + 3):
    """Values spread over binades (the FakeEngine distribution of tests/test_fedavg_dist.py)."""
    g = torch.Generator().manual_seed(100 + seed)
    p16 = torch.randn(n16, generator=g).half()
    p32 = torch.randn(n32, generator=g) * torch.exp2(torch.randint(-6, 6, (n32,), generator=g).float())
    return p16, p32


def weighted_reference(clients, weights):
    acc = ws = None
    for (p16, p32), w in zip(clients, weights):
        x = torch.cat([p16.float(), p32])
        wt = torch.tensor(float(w), dtype=torch.float32)
        if acc is None:
            acc, ws = wt * x, wt.clone()
        else:
            acc += wt * x
            ws += wt
    v = (acc / ws).half()
    n16 = clients[0][0].numel()
    return v[:n16], v[n16:].float()


def test_pack_and_unpack_weighted_kernels(dev):
    p16, p32 = _client(0)
    n16, n32 = p16.numel(), p32.numel()
    n = n16 + n32
    d16, d32 = p16.to(dev), p32.to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    bucket = torch.full((n + 2,), -7.0, device=dev)
    ops.fedavg_pack_weighted(d16, d32, flag, 3.0, bucket)
    w = torch.tensor(3.0)
    host = torch.cat([w * p16.float(), w * p32, torch.tensor([3.0, 1.0])])
    assert torch.equal(bucket.cpu(), host)
    # the sum of one client: fp16(bucket[i] / bucket[n]), kept as the global copy too
    o16, o32 = torch.zeros_like(d16), torch.zeros_like(d32)
    g16, g32 = torch.ones_like(d16), torch.ones_like(d32)
    ops.fedavg_unpack_weighted(bucket, o16, o32, g16, g32)
    v = (host[:n] / host[n]).half()
    assert torch.equal(o16.cpu(), v[:n16]) and torch.equal(o32.cpu(), v[n16:].float())
    assert torch.equal(g16, o16) and torch.equal(g32, o32)
    # a set flag: all zeros, the weight and the vote included
    flag.fill_(1)
    bucket.fill_(-7.0)
    ops.fedavg_pack_weighted(d16, d32, flag, 3.0, bucket)
    assert torch.equal(bucket.cpu(), torch.zeros(n + 2))
    # no vote: the trainables go back to the global copy, which stays
    prev16, prev32 = g16.clone(), g32.clone()
    o16.fill_(5.0)
    o32.fill_(5.0)
    ops.fedavg_unpack_weighted(bucket, o16, o32, g16, g32)
    assert torch.equal(o16, prev16) and torch.equal(o32, prev32)
    assert torch.equal(g16, prev16) and torch.equal(g32, prev32)
    # argument validation, as the siblings': sizes, dtypes, the weight
    with pytest.raises((ValueError, AssertionError)):
        ops.fedavg_pack_weighted(d16, d32, flag, 3.0, bucket[:n + 1])
    with pytest.raises(ValueError):
        ops.fedavg_pack_weighted(d16, d32, flag, 0.0, bucket)
    with pytest.raises(ValueError):
        ops.fedavg_pack_weighted(d16.float(), d32, flag, 3.0, bucket)


def test_plain_and_unit_weight_chains_agree(dev):
    """The plain and the weighted pack / unpack kernels are two instantiations of one body: with every weight 1.0
    (1.0f * x is exact; the summed weights and the vote count are both 3.0f) pack x 3 -> reduce_ordered -> unpack
    gives the plain chain's p16, p32, g16, g32 bit for bit, and the plain chain equals torch's
    acc = x0; acc += x1; acc += x2; (acc / 3).half().  Ragged n16 = 37, n32 = 4099: the n16 split sits mid-block."""
    clients = [_client(c) for c in range(3)]
    n16, n32 = clients[0][0].numel(), clients[0][1].numel()
    n = n16 + n32
    dclients = [(p16.to(dev), p32.to(dev)) for p16, p32 in clients]
    prev16 = torch.full((n16,), 0.5, dtype=torch.float16, device=dev)
    prev32 = torch.full((n32,), 0.25, device=dev)

    def chain(weighted, invalid):
        tail = 2 if weighted else 1
        gathered = torch.empty(3, n + tail, device=dev)
        for c, (p16, p32) in enumerate(dclients):
            flag = torch.full((1,), int(c in invalid), dtype=torch.int32, device=dev)
            if weighted:
                ops.fedavg_pack_weighted(p16, p32, flag, 1.0, gathered[c])
            else:
                ops.fedavg_pack(p16, p32, flag, gathered[c])
        total = torch.empty(n + tail, device=dev)
        ops.fedavg_reduce_ordered(gathered.view(-1), 3, total)
        assert all(t.item() == 3.0 - len(invalid) for t in total[n:])
        o16, o32 = torch.full_like(prev16, 5.0), torch.full_like(prev32, 5.0)
        g16, g32 = prev16.clone(), prev32.clone()
        (ops.fedavg_unpack_weighted if weighted else ops.fedavg_unpack)(total, o16, o32, g16, g32)
        return o16, o32, g16, g32

    def host_mean(which):
        xs = [torch.cat([clients[c][0].float(), clients[c][1]]) for c in which]
        acc = xs[0].clone()
        for x in xs[1:]:
            acc += x
        v = (acc / len(which)).half()
        return v[:n16], v[n16:].float()

    for invalid, which in (((), (0, 1, 2)), ((1,), (0, 2))):
        plain, weighted = chain(False, invalid), chain(True, invalid)
        ref16, ref32 = host_mean(which)
        assert torch.equal(plain[0].cpu(), ref16) and torch.equal(plain[1].cpu(), ref32)
        assert torch.equal(plain[2], plain[0]) and torch.equal(plain[3], plain[1])  # kept as the global copy
        for a, b in zip(plain, weighted):
            assert torch.equal(a, b)
    # the invalid client changed the mean
    assert not torch.equal(host_mean((0, 1, 2))[1], host_mean((0, 2))[1])
    # all three invalid: both chains restore the previous global copy, which stays
    for weighted in (False, True):
        o16, o32, g16, g32 = chain(weighted, (0, 1, 2))
        assert torch.equal(o16, prev16) and torch.equal(o32, prev32)
        assert torch.equal(g16, prev16) and torch.equal(g32, prev32)


def test_weighted_pack_reduce_unpack_chain_is_bit_exact(dev):
    clients = [_client(c) for c in range(3)]
    weights = (3.0, 1.0, 2.0)
    n16, n32 = clients[0][0].numel(), clients[0][1].numel()
    n = n16 + n32
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    gathered = torch.empty(3, n + 2, device=dev)
    for c, ((p16, p32), w) in enumerate(zip(clients, weights)):
        ops.fedavg_pack_weighted(p16.to(dev), p32.to(dev), flag, w, gathered[c])
    total = torch.empty(n + 2, device=dev)
    ops.fedavg_reduce_ordered(gathered.view(-1), 3, total)
    assert total[n].item() == 6.0 and total[n + 1].item() == 3.0
    o16 = torch.empty(n16, dtype=torch.float16, device=dev)
    o32 = torch.empty(n32, device=dev)
    ops.fedavg_unpack_weighted(total, o16, o32)
    ref16, ref32 = weighted_reference(clients, weights)
    assert torch.equal(o16.cpu(), ref16) and torch.equal(o32.cpu(), ref32)
    # the weights matter: the unweighted mean of the same clients differs
    plain = (torch.stack([p32 for _, p32 in clients]).sum(0) / 3).half().float()
    assert (plain != ref32).float().mean().item() > 0.5


# ----------------------------------------------------------------------------- proximal SGD kernels

def _rt(x, T):
    return x.to(T).float()


def host_prox_step(p, g, buf, q, coef, lr, mom, wd, mu, first):
    """The proximal step op by op on the host (CPU tensors of dtype T in, (p, g, buf) of dtype T out):
    gc = T(g*coef); d = T(p - q); gp = T(gc + mu*d); dp = T(gp + wd*p); b = dp | T(T(buf*mom) + dp);
    p = T(p - lr*b).  Scalars in fp32; every product and sum is one fp32 torch op (no fused multiply-add)."""
    T = p.dtype
    f = lambda v: torch.as_tensor(v, dtype=torch.float32)
    pf = p.float()
    gc = _rt(g.float() * f(coef), T)
    d = _rt(pf - q.float(), T)
    gp = _rt(gc + f(mu) * d, T)
    dp = _rt(gp + f(wd) * pf, T)
    b = dp if first else _rt(_rt(buf.float() * f(mom), T) + dp, T)
    pn = _rt(pf + f(-lr) * b, T)
    return pn.to(T), gc.to(T), b.to(T)


def _ulp16(ref):
    return torch.exp2(torch.floor(torch.log2(ref.float().abs().clamp_min(2.0 ** -14))) - 10)


SIZES = {"vector": (10000, 5000, 0), "scalar": (10003, 5005, 0), "offset": (10000, 5000, 1)}


class _State:
    """p, pglob and two steps' gradients of one case, on the host; device() makes fresh device copies, each buffer
    a slice starting `off` elements into a 256-byte-aligned allocation (off = 1: the unaligned fallback).

    |p| >= 2^-4: the kernels' results are compared with references within one fp16 ulp of p and of buf; a
    one-ulp difference of buf (|buf| < 0.25 here, ulp <= 2^-13) moves p by lr * 2^-13 = 1.2e-5, which stays inside
    one ulp of p only when ulp(p) >= 2^-14, i.e. |p| >= 2^-4.  Nearer zero the bound on p would not follow from the
    bound on buf."""

    def __init__(self, case, seed=0):
        self.n16, self.n32, self.off = SIZES[case]
        gen = torch.Generator().manual_seed(seed)

        def weights(n):
            p = torch.randn(n, generator=gen)
            return p + 0.0625 * torch.sign(p)

        self.p16, self.p32 = weights(self.n16).half(), weights(self.n32)
        self.q16 = (self.p16.float() + 0.05 * torch.randn(self.n16, generator=gen)).half()
        self.q32 = self.p32 + 0.05 * torch.randn(self.n32, generator=gen)
        self.grads = [((torch.randn(self.n16, generator=gen) * 0.05).half(),
                       torch.randn(self.n32, generator=gen) * 0.05) for _ in range(2)]

    def _dev(self, t, dev):
        base = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev)
        view = base[self.off:self.off + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 32 == (self.off * t.element_size()) % 32
        return view

    def device(self, dev, same_global=False):
        d = {k: self._dev(getattr(self, k), dev) for k in ("p16", "p32", "q16", "q32")}
        if same_global:
            d["q16"].copy_(d["p16"])
            d["q32"].copy_(d["p32"])
        d["b16"], d["b32"] = self._dev(torch.zeros_like(self.p16), dev), self._dev(torch.zeros_like(self.p32), dev)
        d["g16"], d["g32"] = self._dev(self.grads[0][0], dev), self._dev(self.grads[0][1], dev)
        return d

    def chunks(self, dev):
        ce = ops.optim_chunk_elems()
        rows = [(sid, is16, s, min(n, s + ce)) for sid, is16, n in ((0, 1, self.n16), (1, 0, self.n32))
                for s in range(0, n, ce)]
        arr = np.zeros(len(rows), dtype=np.dtype([("seg", np.int32), ("is16", np.int32), ("s", np.int64),
                                                  ("e", np.int64)]))
        for i, r in enumerate(rows):
            arr[i] = r
        return torch.from_numpy(arr.view(np.uint8)).to(dev), len(rows)


def _run(st, dev, api, mu, prox=True, steps=1, halt=0.0, same_global=False):
    """`steps` optimizer steps on fresh device copies; returns the device buffers and the clip outputs per step.
    prox=False: the existing ops.sgd_step / ops.optimizer_step on the same inputs."""
    d = st.device(dev, same_global)
    chunks, nchunks = st.chunks(dev)
    part = torch.empty(nchunks, device=dev)
    out = torch.empty(3, device=dev)
    hyper = torch.tensor([LR, MOM, WD, 1.0, halt, mu], device=dev)
    halt_src = torch.zeros(1, device=dev)
    coefs = []
    for s in range(steps):
        if s:
            d["g16"].copy_(st.grads[s][0])
            d["g32"].copy_(st.grads[s][1])
            hyper[3] = 0.0
        if api == "fused":
            args = (d["p16"], d["g16"], d["b16"], d["p32"], d["g32"], d["b32"], chunks, nchunks, 1.0, part, out,
                    hyper, halt_src, None)
            if prox:
                ops.optimizer_step_prox(*args, d["q16"], d["q32"])
            else:
                ops.optimizer_step(*args)
        else:
            ops.clip_grad_norm(d["g16"], d["g32"], chunks, nchunks, 1.0, part, out)
            for k in ("16", "32"):
                if prox:
                    ops.sgd_prox_step(d["p" + k], d["g" + k], d["b" + k], d["q" + k], out, hyper)
                else:
                    ops.sgd_step(d["p" + k], d["g" + k], d["b" + k], out, hyper)
        coefs.append(out[1].item())
    torch.cuda.synchronize()
    return d, coefs


CASES = [(c, a) for c in SIZES for a in ("step", "fused")]
KEYS = ("p16", "g16", "b16", "p32", "g32", "b32")


@pytest.fixture(scope="module")
def states():
    return {c: _State(c) for c in SIZES}


@pytest.mark.parametrize("case,api", CASES)
def test_prox_mu_zero_is_the_plain_step_bit_for_bit(dev, states, case, api):
    """GPU against GPU, two steps (first-step and momentum paths)."""
    st = states[case]
    a, _ = _run(st, dev, api, 0.0, prox=True, steps=2)
    b, _ = _run(st, dev, api, 0.0, prox=False, steps=2)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["p16"].cpu(), st.p16)  # a step was taken


@pytest.mark.parametrize("case,api", CASES)
def test_prox_term_is_exactly_zero_at_the_global_weights(dev, states, case, api):
    st = states[case]
    a, _ = _run(st, dev, api, 0.5, same_global=True)
    b, _ = _run(st, dev, api, 0.0, same_global=True)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case,api", CASES)
def test_prox_halt_leaves_everything_untouched(dev, states, case, api):
    st = states[case]
    d, _ = _run(st, dev, api, 0.5, halt=1.0)
    assert torch.equal(d["p16"].cpu(), st.p16) and torch.equal(d["p32"].cpu(), st.p32)
    assert torch.equal(d["g16"].cpu(), st.grads[0][0]) and torch.equal(d["g32"].cpu(), st.grads[0][1])
    assert not d["b16"].any() and not d["b32"].any()


@pytest.mark.parametrize("case,api", CASES)
def test_prox_step_equals_the_host_restatement(dev, states, case, api):
    """Two steps at mu = 0.5 against host_prox_step fed the device's own clip coefficient: IEEE fp32 operations in
    the same order with the same roundings on both sides, so bit for bit -- p, the stored (clipped) gradient and
    the momentum, fp16 and fp32."""
    st = states[case]
    d, coefs = _run(st, dev, api, 0.5, steps=2)
    h = {"p16": st.p16, "p32": st.p32, "b16": torch.zeros_like(st.p16), "b32": torch.zeros_like(st.p32)}
    for s in range(2):
        for k, q in (("16", st.q16), ("32", st.q32)):
            h["p" + k], h["g" + k], h["b" + k] = host_prox_step(h["p" + k], st.grads[s][k == "32"], h["b" + k], q,
                                                                coefs[s], LR, MOM, WD, 0.5, s == 0)
    for k in KEYS:
        assert torch.equal(d[k].cpu(), h[k]), k


@pytest.mark.parametrize("case,api", CASES)
def test_prox_step_against_torch_sgd_on_the_cpu(dev, states, case, api):
    """mu = 0.5, lr = 0.1, two steps, against torch on the CPU: clip_grad_norm_, grad.add_(p - pglob, alpha=mu),
    torch.optim.SGD(foreach=False).  Bounds: every fp16 element of p and of buf within one fp16 ulp of the
    reference, at most 1 % of them unequal, fp32 within rtol 1e-6 / atol 1e-7.

    lr and weight decay are the fp16-exact LR / WD above, so that torch's CPU arithmetic (which rounds the alpha of
    add() to fp16 for Half tensors) and the kernels (fp32 scalars) step with the same numbers; with lr = 0.1 and
    weight decay = 5e-4 as doubles the two sides would run different hyper-parameters (measured on the MI355X
    then: momentum up to 128 ulp away, 3.0-3.3 % unequal).  What is left between them is torch's fused
    multiply-adds: the host restatement against this reference, CPU only, seeds 0-3: at most one ulp, at most
    0.02 % of the fp16 elements unequal.  Measured on the MI355X with the inputs below: vector and offset, p16 and
    b16 equal to the reference; scalar, one element of p16 one ulp away (0.010 %), b16 equal; p32 within 1.2e-7 and
    b32 within 6e-8 absolute; both entry points alike."""
    mu = 0.5
    st = states[case]
    d, _ = _run(st, dev, api, mu, steps=2)
    d0, _ = _run(st, dev, api, 0.0, steps=2)
    rp16, rp32 = st.p16.clone().requires_grad_(True), st.p32.clone().requires_grad_(True)
    opt = torch.optim.SGD([rp16, rp32], lr=LR, momentum=MOM, weight_decay=WD, foreach=False)
    for s in range(2):
        rp16.grad, rp32.grad = st.grads[s][0].clone(), st.grads[s][1].clone()
        torch.nn.utils.clip_grad_norm_([rp16, rp32], 1.0)
        rp16.grad.add_(rp16.detach() - st.q16, alpha=mu)
        rp32.grad.add_(rp32.detach() - st.q32, alpha=mu)
        opt.step()
    ref = {"p16": rp16.detach(), "p32": rp32.detach(), "b16": opt.state[rp16]["momentum_buffer"],
           "b32": opt.state[rp32]["momentum_buffer"]}
    fig = {}
    for k in ("p16", "b16"):
        got = d[k].cpu()
        fig[k] = (((got.float() - ref[k].float()).abs() / _ulp16(ref[k])).max().item(),
                  (got != ref[k]).float().mean().item())
        print(f"{case}/{api} {k}: max {fig[k][0]:.2f} ulp, {100 * fig[k][1]:.3f} % unequal")
    for k in ("p32", "b32"):
        print(f"{case}/{api} {k}: max |diff| {(d[k].cpu() - ref[k]).abs().max().item():.3e}")
    # the test can fail: the proximal term changes most of the momentum buffer
    assert (d["b16"] != d0["b16"]).float().mean().item() > 0.5
    assert (d["b32"] != d0["b32"]).float().mean().item() > 0.5
    for k in ("p32", "b32"):
        torch.testing.assert_close(d[k].cpu(), ref[k], rtol=1e-6, atol=1e-7)
    for k in ("p16", "b16"):
        assert fig[k][0] <= 1.0 and fig[k][1] <= 0.01, (k, fig[k])


def test_prox_argument_validation(dev):
    n = 64
    p, g, b, q = (torch.zeros(n, dtype=torch.float16, device=dev) for _ in range(4))
    out = torch.ones(3, device=dev)
    hyper5 = torch.tensor([LR, MOM, WD, 1.0, 0.0], device=dev)
    hyper6 = torch.tensor([LR, MOM, WD, 1.0, 0.0, 0.5], device=dev)
    with pytest.raises(ValueError):
        ops.sgd_prox_step(p, g, b, q, out, hyper5)        # mu lives at hyper[5]
    with pytest.raises(ValueError):
        ops.sgd_prox_step(p, g, b, q.float(), out, hyper6)
    with pytest.raises(ValueError):
        ops.sgd_prox_step(p, g, b, q[:32], out, hyper6)
    with pytest.raises(ValueError):
        ops.sgd_prox_step(p, g, b, p, out, hyper6)        # the global copy is a buffer of its own
    ops.sgd_prox_step(p, g, b, q, out, hyper6)


# ----------------------------------------------------------------------------- through the trainer

def small_cfg(out, clients=2, rounds=1, epochs=1, extra=()):
    """small_cfg of tests/test_trainers_gpu.py: ViT-B/16, batch 4, 10 classes, J = 3."""
    cfg = get_cfg_default()
    extend_cfg(cfg)
    cfg.merge_from_file("configs/trainers/MaPLeFederated/vit_b16_c2_ep5_batch4_2ctx_cross_datasets.yaml")
    cfg.merge_from_list(["TRAINER.NAME", "MaPLeFederated", "SEED", 1, "OUTPUT_DIR", str(out),
                         "FED.NUM_CLIENTS", clients, "FED.NUM_ROUNDS", rounds, "FED.LOCAL_EPOCHS", epochs,
                         "MODEL.NUM_CLASSES", 10, "DATASET.NUM_SHOTS", 1, "DATALOADER.TEST.BATCH_SIZE", 12,
                         "TRAINER.MAPLE.PROMPT_DEPTH", 3] + list(extra))
    cfg.freeze()
    return cfg


def test_proximal_trainer_beside_a_plain_one(dev, tmp_path):
    # the config's warm-up learning rate (1e-4) moves hardly any fp16 weight in one step; 0.01 moves many, so the
    # proximal term is non-zero in the fp16 buffer too at step 2
    lr = ["OPTIM.WARMUP_CONS_LR", 0.01]
    prox = build_trainer(small_cfg(tmp_path / "prox", extra=["FED.PROX_MU", 0.5] + lr))
    plain = build_trainer(small_cfg(tmp_path / "plain", extra=lr))
    ca, cb = prox.clients[0], plain.clients[0]
    ea, eb = ca.engine, cb.engine
    assert ea._prox["glob"] is not None and eb._prox["glob"] is None
    assert ea._prox["glob"][0] is prox.fed[0].global16 and ea.hyper[5].item() == 0.5
    batch = next(iter(cb.dm.train_loader))
    # step 1 (eager, first_step): the weights equal the global copy, so the term is exactly zero
    ca.forward_backward(batch)
    cb.forward_backward(batch)
    for k in ("flat16", "flat32", "mom16", "mom32", "gflat16", "gflat32"):
        assert torch.equal(getattr(ea, k), getattr(eb, k)), k
    # step 2 (the captured graph, momentum path): the weights have left the global copy
    p_before, b_before = ea.flat16.clone(), ea.mom16.clone()
    p32_before, b32_before = ea.flat32.clone(), ea.mom32.clone()
    assert not torch.equal(p_before, prox.fed[0].global16) and not torch.equal(p32_before, prox.fed[0].global32)
    ca.forward_backward(batch)
    cb.forward_backward(batch)
    assert ca._graphs and ea._prox["captured"]
    assert not torch.equal(ea.flat32, eb.flat32) and not torch.equal(ea.mom32, eb.mom32)
    assert not torch.equal(ea.mom16, eb.mom16)
    # the momentum the captured step left == the restatement on the step's own operands: the weights and momentum
    # before it, the clipped gradient it stored back (coefficient 1 from here) and the bucket's global copy
    lr, mom, wd, first, halt, mu = ea.hyper.tolist()
    assert first == 0.0 and halt == 0.0 and mu == 0.5
    fed = prox.fed[0]
    _, _, want = host_prox_step(p_before.cpu(), ea.gflat16.cpu(), b_before.cpu(), fed.global16.cpu(), 1.0, lr, mom,
                                wd, mu, False)
    got = ea.mom16.cpu()
    assert ((got.float() - want.float()).abs() <= _ulp16(want)).all()
    assert (got != want).float().mean().item() <= 0.01
    _, _, want32 = host_prox_step(p32_before.cpu(), ea.gflat32.cpu(), b32_before.cpu(), fed.global32.cpu(), 1.0, lr,
                                  mom, wd, mu, False)
    torch.testing.assert_close(ea.mom32.cpu(), want32, rtol=1e-6, atol=1e-7)
    # ... and not the restatement with the weights themselves in the global copy's place: the copy was read
    _, _, without = host_prox_step(p_before.cpu(), ea.gflat16.cpu(), b_before.cpu(), p_before.cpu(), 1.0, lr, mom, wd,
                                   mu, False)
    assert not torch.equal(want, without) and (got != without).sum().item() >= (want != without).sum().item() // 2
    with pytest.raises(RuntimeError):
        ea.set_proximal(0.5, prox.fed[0].global16, prox.fed[0].global32)  # a step is captured
    ea.set_prox_mu(0.25)  # ... while mu itself is device memory
    assert ea.hyper[5].item() == 0.25
    # FedAvg refreshes the global copy in place: every client is back at it
    assert prox._fedavg([]) == 2
    for c, fed in zip(prox.clients, prox.fed):
        assert torch.equal(fed.global16, c.engine.flat16) and torch.equal(fed.global32, c.engine.flat32)
        assert c.engine._prox["glob"][0] is fed.global16 and c.engine._prox["glob"][1] is fed.global32
    with pytest.raises(ValueError):
        build_trainer(small_cfg(tmp_path / "neg", extra=["FED.PROX_MU", -0.1]))


def test_weighted_trainer(dev, tmp_path):
    tr = build_trainer(small_cfg(tmp_path, clients=3, extra=["FED.CLIENT_WEIGHTS", "3,1,2"]))
    assert tr.client_weights == [3.0, 1.0, 2.0] and [f.weight for f in tr.fed] == [3.0, 1.0, 2.0]
    for c in tr.clients:
        c.run_epoch(0)
    names = tr.clients[0].engine.trainable_names
    snaps = [{n: c.engine.P[n].detach().clone().cpu() for n in names} for c in tr.clients]
    flats = [(c.engine.flat16.clone(), c.engine.flat32.clone()) for c in tr.clients]
    assert not all(torch.equal(snaps[0][n], snaps[i][n]) for n in names for i in (1, 2))

    def restatement(which, weights):
        acc = {n: torch.tensor(weights[0]) * snaps[which[0]][n].float() for n in names}
        ws = torch.tensor(weights[0])
        for c, w in zip(which[1:], weights[1:]):
            for n in names:
                acc[n] += torch.tensor(w) * snaps[c][n].float()
            ws = ws + torch.tensor(w)
        return {n: (acc[n] / ws).half() for n in names}

    assert tr._fedavg([]) == 3
    ref = restatement((0, 1, 2), (3.0, 1.0, 2.0))
    for n in names:
        for c in tr.clients:
            assert torch.equal(c.engine.P[n].detach().cpu().float(), ref[n].float()), n
    # the host form of the same mean
    host = tr.safe_average_weights(snaps, weights=tr.client_weights)
    assert all(torch.equal(host[n], ref[n]) for n in names)
    # the same local results again, client 1 invalid: the (3, 2)-weighted mean of the other two
    for c, (f16, f32) in zip(tr.clients, flats):
        c.engine.flat16.copy_(f16)
        c.engine.flat32.copy_(f32)
    tr.clients[1].engine.flat32[0] = float("nan")
    assert tr._fedavg([]) == 2
    ref = restatement((0, 2), (3.0, 2.0))
    for n in names:
        for c in tr.clients:
            assert torch.equal(c.engine.P[n].detach().cpu().float(), ref[n].float()), n


def test_full_round_with_both_options(dev, tmp_path):
    tr = build_trainer(small_cfg(tmp_path, extra=["FED.CLIENT_WEIGHTS", "samples", "FED.PROX_MU", 0.5]))
    n = tr.clients[0].dm.train_loader.s.labels.numel()
    assert tr.client_weights == [float(n), float(n)]
    tr.train()
    assert tr.nan_stats["total_updates"] == 1 and tr.nan_stats["skipped_rounds"] == 0
    for c, fed in zip(tr.clients, tr.fed):
        assert torch.equal(fed.global16, c.engine.flat16) and torch.equal(fed.global32, c.engine.flat32)
