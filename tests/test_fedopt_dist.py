"""CPU tier: the FedOpt server optimizers (FED.SERVER_OPT: FedAvgM, Hsu et al. 2019; FedAdagrad / FedAdam / FedYogi,
Reddi et al., ICLR 2021, Algorithm 2) through federated.ServerOptimizer and the collective protocol of
federated_multi_modal_amd/federated.py on gloo ranks, with host restatements of mf_fedopt_step / mf_fedopt_deliver
in the kernels' place (the GPU tier, tests/test_fedopt_gpu.py, checks the kernels against the same restatements bit
for bit).

host_step is the restatement: torch fp32 on the CPU, one torch op per rounding point of the kernel, the scalars as
fp32 tensors, 1 - beta formed in fp32.  Everything else here compares with it bit for bit;
test_restatement_against_fp64_and_spot_values ties it to the papers' formulas."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_fedavg_dist import FakeEngine, _init, _spawn
from test_fedavg_weighted_dist import WeightedHostKernels

OPTS = ("fedavgm", "fedadagrad", "fedadam", "fedyogi")
# values fp32 does not hold exactly, so the fp32 rounding of the scalars themselves is part of what is compared
HP = {"lr": 0.1, "beta1": 0.9, "beta2": 0.99, "tau": 1e-3}
N16, N32 = 37, 4096 + 3


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def host_step(opt, total, d, x, m, v, lr, beta1, beta2, tau):
    """One server step on fp32 CPU tensors: total = the summed bucket's n values, d = its divisor (the vote count or
    the summed weights, a 0-dim fp32 tensor).  Returns the new (x, m, v); v is passed through for fedavgm."""
    b1, b2, ta, eta, one = _f(beta1), _f(beta2), _f(tau), _f(lr), _f(1.0)
    mean = total / d
    delta = mean - x
    if opt == "fedavgm":
        m = b1 * m + delta
        upd = m
    else:
        m = b1 * m + (one - b1) * delta
        s = delta * delta
        if opt == "fedadagrad":
            v = v + s
        elif opt == "fedadam":
            v = b2 * v + (one - b2) * s
        elif opt == "fedyogi":
            v = v - ((one - b2) * s) * torch.sign(v - s)
        else:
            raise ValueError(opt)
        upd = m / (sqrt32(v) + ta)
    return x + eta * upd, m, v


def sqrt32(v):
    """The correctly rounded fp32 square root (IEEE 754, what sqrtf is on the device).  torch.sqrt is not it on
    every CPU: the AVX-512 build of torch 2.10 vectorises it through an approximation that is one ulp away on 0.6 %
    of fp32 values (and in fp64 alike), which showed as 43 of 4136 elements of x differing from the MI355X in
    FedAdagrad's first round.  numpy's fp32 sqrt is the hardware instruction; test_sqrt32_is_correctly_rounded pins
    it against the fp64 root rounded once more (exact for square roots: 53 >= 2 * 24 + 2 bits)."""
    return torch.from_numpy(np.sqrt(v.detach().contiguous().numpy()))


class FedOptHostKernels(WeightedHostKernels):
    """The host kernels plus the server step and deliver, with ops.fedopt_step's / ops.fedopt_deliver's signatures."""
    steps = 0  # per process: how many times the step ran

    @staticmethod
    def _write(x, p16, p32, g16, g32):
        n16 = p16.numel()
        val = x.half()
        p16.copy_(val[:n16])
        p32.copy_(val[n16:].float())
        g16.copy_(p16)
        g32.copy_(p32)

    @classmethod
    def fedopt_step(cls, bucket, weighted, opt, beta1, beta2, tau, eta, x, m, v, p16, p32, g16, g32):
        cls.steps += 1
        n = p16.numel() + p32.numel()
        if float(bucket[n + int(bool(weighted))]) == 0:
            p16.copy_(g16)
            p32.copy_(g32)
            return
        xn, mn, vn = host_step(opt, bucket[:n], bucket[n], x, m, v, eta, beta1, beta2, tau)
        x.copy_(xn)
        m.copy_(mn)
        if v is not None:
            v.copy_(vn)
        cls._write(x, p16, p32, g16, g32)

    @classmethod
    def fedopt_deliver(cls, x, p16, p32, g16, g32):
        cls._write(x, p16, p32, g16, g32)


def _engine():
    """The previous global weights, identical on every rank: FakeEngine's values spread over binades."""
    return FakeEngine(0, n16=N16, n32=N32)


def local_result(client, rnd, g16, g32):
    """Client `client`'s weights after its local training of round `rnd`, from the global weights it was given: a
    deterministic update whose size differs per round (2^-3, 2^-8, 1 times the weight, plus an absolute part)."""
    g = torch.Generator().manual_seed(7000 + 100 * rnd + client)
    scale = (2.0 ** -3, 2.0 ** -8, 1.0)[rnd % 3]
    p16 = (g16.float() + scale * 0.5 * torch.randn(g16.numel(), generator=g)).half()
    p32 = g32 + scale * (torch.randn(g32.numel(), generator=g) * g32.abs() + 1e-3 * torch.randn(g32.numel(), generator=g))
    return p16, p32


class Replay:
    """The single-process restatement of the rounds: the clients' results summed in client order (weighted: fp32
    products w * x, then the sums), one host_step per round with a valid client, the fp16 rounding delivered."""

    def __init__(self, opt, hp=HP, weights=None):
        e = _engine()
        self.opt, self.hp, self.weights = opt, hp, weights
        self.g16, self.g32 = e.flat16.clone(), e.flat32.clone()
        self.x = torch.cat([self.g16.float(), self.g32])
        self.m = torch.zeros_like(self.x)
        self.v = None if opt == "fedavgm" else torch.full_like(self.x, float(_f(hp["tau"]) * _f(hp["tau"])))

    def round(self, clients, rnd, results=None):
        """clients: the valid clients' ids, in client order.  results: {client: (p16, p32)} to use instead of
        local_result."""
        if not clients:
            return
        acc = ws = None
        for c in clients:
            p16, p32 = results[c] if results is not None else local_result(c, rnd, self.g16, self.g32)
            xc = torch.cat([p16.float(), p32])
            if self.weights is None:
                acc = xc.clone() if acc is None else acc + xc
                ws = _f(1.0) if ws is None else ws + _f(1.0)
            else:
                w = _f(self.weights[c])
                acc = w * xc if acc is None else acc + w * xc
                ws = w.clone() if ws is None else ws + w
        self.x, self.m, self.v = host_step(self.opt, acc, ws, self.x, self.m, self.v, **self.hp)
        val = self.x.half()
        self.g16, self.g32 = val[:N16].clone(), val[N16:].float()

    def state(self):
        return (self.g16, self.g32, self.g16, self.g32, self.x, self.m, self.v)


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def _state(e, fed, server):
    cl = lambda t: None if t is None else t.clone()  # noqa: E731
    return (cl(e.flat16), cl(e.flat32), cl(fed.global16), cl(fed.global32), cl(server.x), cl(server.m), cl(server.v))


NAMES = ("p16", "p32", "g16", "g32", "x", "m", "v")


def _assert_state(got, want, what=""):
    for k, a, b in zip(NAMES, got, want):
        assert _same(a, b), f"{what} {k}"


# ----------------------------------------------------------------------------- 1. the restatement itself

def fp64_reference(opt, x0, rounds, lr, beta1, beta2, tau):
    """Hsu et al.'s server momentum and Reddi et al.'s Algorithm 2 (no bias correction) in numpy fp64, written from
    the papers: Delta_t = mean of the clients - x_t; FedAvgM m_t = beta1 m_{t-1} + Delta_t, x_{t+1} = x_t + eta m_t;
    adaptive m_t = beta1 m_{t-1} + (1 - beta1) Delta_t, v_t = v_{t-1} + Delta_t^2 | beta2 v_{t-1} + (1 - beta2)
    Delta_t^2 | v_{t-1} - (1 - beta2) Delta_t^2 sign(v_{t-1} - Delta_t^2), x_{t+1} = x_t + eta m_t / (sqrt(v_t) + tau),
    v_{-1} = tau^2.  The hyper-parameters are the fp32 values the kernel is handed, so that the comparison measures
    the arithmetic and not the rounding of 0.9 to fp32."""
    lr, b1, b2, tau = (np.float64(np.float32(h)) for h in (lr, beta1, beta2, tau))
    x = x0.double().numpy().copy()
    m = np.zeros_like(x)
    v = np.full_like(x, tau * tau)
    for clients in rounds:
        mean = np.sum([c.double().numpy() for c in clients], axis=0) / len(clients)
        delta = mean - x
        if opt == "fedavgm":
            m = b1 * m + delta
            x = x + lr * m
            continue
        m = b1 * m + (1.0 - b1) * delta
        d2 = delta ** 2
        if opt == "fedadagrad":
            v = v + d2
        elif opt == "fedadam":
            v = b2 * v + (1.0 - b2) * d2
        else:
            v = v - (1.0 - b2) * d2 * np.sign(v - d2)
        x = x + lr * m / (np.sqrt(v) + tau)
    return x


# the largest deviation of the fp32 restatement's x from the fp64 statement after three rounds, relative to
# |x| + eta * tau, measured over the inputs of _fp64_inputs on an x86-64 host: see the test's docstring.  The gate
# is twice that: another round's inputs reorder the roundings but do not change their number.
FP64_MEASURED = {"fedavgm": 5.24e-7, "fedadagrad": 5.54e-5, "fedadam": 8.23e-5, "fedyogi": 8.10e-5}


def _fp64_inputs():
    g = torch.Generator().manual_seed(11)
    n = 4096
    x0 = (torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 6, (n,), generator=g).float())).half().float()
    rounds = []
    for scale in (2.0 ** -3, 2.0 ** -8, 1.0):  # rounds of differing Delta
        rounds.append([x0 * (1.0 + scale * torch.randn(n, generator=g)) + scale * 1e-2 * torch.randn(n, generator=g)
                       for _ in range(3)])
    return x0, rounds


@pytest.mark.parametrize("opt", OPTS)
def test_restatement_against_fp64_and_spot_values(opt):
    """host_step over three rounds against fp64_reference, 4096 values spread over twelve binades, three clients,
    rounds whose Delta differ in size by 2^8.  Measured deviation of x, max over the elements of
    |x32 - x64| / (|x64| + eta * tau):
        fedavgm 5.24e-7, fedadagrad 5.54e-5, fedadam 8.23e-5, fedyogi 8.10e-5   (FP64_MEASURED; medians 3e-8 to 7e-8)
    and the gate is twice the measured value.  The adaptive optimizers sit higher because
    they divide m by sqrt(v), both of the size of Delta = mean - x: where the clients moved little (|Delta| down to
    2^-8 |x| here) the subtraction cancels, Delta carries a relative error of eps * |x| / |Delta|, and the
    normalised update hands it to x at the scale of eta.  The spot values below are worked by hand on
    numbers fp32 holds exactly (so every intermediate is exact): they are what catches a wrong formula that the
    kernel and the restatement would share."""
    x0, rounds = _fp64_inputs()
    ref = fp64_reference(opt, x0, rounds, **HP)
    x, m = x0.clone(), torch.zeros_like(x0)
    v = None if opt == "fedavgm" else torch.full_like(x0, float(_f(HP["tau"]) * _f(HP["tau"])))
    for clients in rounds:
        total = clients[0].clone()
        for c in clients[1:]:
            total = total + c
        x, m, v = host_step(opt, total, _f(len(clients)), x, m, v, **HP)
    dev = float(np.max(np.abs(x.double().numpy() - ref) / (np.abs(ref) + HP["lr"] * HP["tau"])))
    print(f"{opt}: fp32 restatement vs fp64, max relative deviation of x {dev:.3e} "
          f"(gate {2 * FP64_MEASURED[opt]:.3e})")
    assert not np.array_equal(ref, x0.double().numpy())
    assert dev <= 2 * FP64_MEASURED[opt]

    one = lambda val: torch.tensor([float(val)])  # noqa: E731
    if opt == "fedavgm":
        # x = 1, mean = 6 / 2 = 3, Delta = 2, m = 0.5 * 2 + 2 = 3, x = 1 + 0.5 * 3 = 2.5
        xs, ms, _ = host_step(opt, one(6), _f(2), one(1), one(2), None, lr=0.5, beta1=0.5, beta2=0.5, tau=2.0)
        assert ms.item() == 3.0 and xs.item() == 2.5
        return
    # x = 1, mean = 3, Delta = 2, s = 4, m = 0.5 * 0 + 0.5 * 2 = 1 in every case below
    if opt == "fedyogi":
        # (1 - beta2) * s = 2; v moves towards s by it: 6 -> 4 (v > s), 2 -> 4 (v < s), 4 -> 4 (v == s: sign 0);
        # sqrt(4) + tau = 4, upd = 0.25, x = 1.25.  A flipped sign would give 8 / 0 / 4.
        for v0 in (6.0, 2.0, 4.0):
            xs, ms, vs = host_step(opt, one(6), _f(2), one(1), one(0), one(v0), lr=1.0, beta1=0.5, beta2=0.5, tau=2.0)
            assert (ms.item(), vs.item(), xs.item()) == (1.0, 4.0, 1.25), v0
    elif opt == "fedadam":
        # v = 0.5 * 28 + 0.5 * 4 = 16, sqrt + tau = 8, upd = 1 / 8
        xs, ms, vs = host_step(opt, one(6), _f(2), one(1), one(0), one(28), lr=1.0, beta1=0.5, beta2=0.5, tau=4.0)
        assert (ms.item(), vs.item(), xs.item()) == (1.0, 16.0, 1.125)
    else:
        # FedAdagrad's v only grows: 5 -> 9 (Delta 2) -> 9 (Delta 0) -> 25 (Delta 4)
        xs, ms, vs = host_step(opt, one(6), _f(2), one(1), one(0), one(5), lr=1.0, beta1=0.5, beta2=0.5, tau=1.0)
        assert (ms.item(), vs.item(), xs.item()) == (1.0, 9.0, 1.25)      # upd = 1 / (3 + 1)
        xs, ms, vs = host_step(opt, one(2.5), _f(2), xs, ms, vs, lr=1.0, beta1=0.5, beta2=0.5, tau=1.0)
        assert (ms.item(), vs.item(), xs.item()) == (0.5, 9.0, 1.375)     # Delta = 0: upd = 0.5 / 4
        xs, ms, vs = host_step(opt, one(10.75), _f(2), xs, ms, vs, lr=1.0, beta1=0.5, beta2=0.5, tau=1.0)
        assert (ms.item(), vs.item(), xs.item()) == (2.25, 25.0, 1.75)    # Delta = 4: m = 0.25 + 2, upd = 2.25 / 6


def test_sqrt32_is_correctly_rounded():
    g = torch.Generator().manual_seed(5)
    v = torch.rand(200_000, generator=g) * torch.exp2(torch.randint(-60, 10, (200_000,), generator=g).float())
    want = np.sqrt(v.double().numpy()).astype(np.float32)
    assert np.array_equal(sqrt32(v).numpy(), want)
    assert sqrt32(torch.tensor([4.0, 9.0, 0.0])).tolist() == [2.0, 3.0, 0.0]


# ----------------------------------------------------------------------------- 2. world sizes 2 and 3

def _bucket(e, opt, weight=None, server=None, hp=HP):
    """A bucket (and, unless one is given, a server optimizer) built while the engine holds the global weights."""
    from federated_multi_modal_amd.federated import FedAvgBucket, ServerOptimizer
    if server is None:
        server = ServerOptimizer(opt, e, **hp)
    return FedAvgBucket(e, kernels=FedOptHostKernels, mode="ordered", weight=weight, server=server), server


def _train(e, fed, client, rnd):
    p16, p32 = local_result(client, rnd, fed.global16, fed.global32)
    e.flat16.copy_(p16)
    e.flat32.copy_(p32)


def _rounds_worker(rank, world, port, weights, out):
    _init(rank, world, port)
    res = {}
    for opt in OPTS:
        e = _engine()
        fed, server = _bucket(e, opt, None if weights is None else weights[rank])
        for rnd in range(2):
            _train(e, fed, rank, rnd)
            assert fed.run() == world
        res[opt] = _state(e, fed, server)
    out[rank] = res
    dist.destroy_process_group()


@pytest.mark.parametrize("world,weights", [(2, None), (3, None), (2, (3, 1)), (3, (3, 1, 2))])
def test_ordered_exchange_two_rounds_bit_exact(world, weights):
    """One client per rank, two consecutive rounds, every optimizer: the weights, the global copy and x, m, v of
    every rank equal the single-process restatement bit for bit (and so each other)."""
    res = _spawn(_rounds_worker, world, weights)
    for opt in OPTS:
        rp = Replay(opt, weights=weights)
        first = Replay(opt, weights=weights)
        first.round(list(range(world)), 0)
        for rnd in range(2):
            rp.round(list(range(world)), rnd)
        assert not torch.equal(rp.x, first.x) and not torch.equal(rp.m, first.m)  # the second round did something
        for r in range(world):
            _assert_state(res[r][opt], rp.state(), f"{opt} rank {r}")
            _assert_state(res[r][opt], res[0][opt], f"{opt} rank {r} vs rank 0")


# ----------------------------------------------------------------------------- 3. two clients per rank

def _group_worker(rank, world, port, per_rank, out):
    _init(rank, world, port)
    from federated_multi_modal_amd.federated import FedAvgExchange
    res = {}
    for opt in OPTS:
        ids = list(range(rank * per_rank, (rank + 1) * per_rank))
        engines = [_engine() for _ in ids]
        server, feds = None, []
        for e in engines:
            fed, server = _bucket(e, opt, server=server)
            feds.append(fed)
        x = FedAvgExchange(feds, mode="ordered")
        before = FedOptHostKernels.steps
        for c, e, fed in zip(ids, engines, feds):
            _train(e, fed, c, 0)
            fed.pack()
        x.start()
        x.finish([])
        for fed in feds:
            fed.unpack()
        res[opt] = ([_state(e, f, server) for e, f in zip(engines, feds)], FedOptHostKernels.steps - before,
                    x.n_valid())
    out[rank] = res
    dist.destroy_process_group()


def test_two_clients_per_rank_step_once():
    res = _spawn(_group_worker, 2, 2)
    for opt in OPTS:
        once = Replay(opt)
        once.round([0, 1, 2, 3], 0)
        for r in range(2):
            states, steps, n_valid = res[r][opt]
            assert steps == 1 and n_valid == 4
            for st in states:  # both local clients: the same delivered bits, the state after one application
                _assert_state(st, once.state(), f"{opt} rank {r}")


# ----------------------------------------------------------------------------- 4.-6. one process

def _local_group(opt, n, hp=HP, weights=None):
    from federated_multi_modal_amd.federated import FedAvgExchange
    engines = [_engine() for _ in range(n)]
    server, feds = None, []
    for c, e in enumerate(engines):
        fed, server = _bucket(e, opt, None if weights is None else weights[c], server, hp)
        feds.append(fed)
    return engines, feds, server, FedAvgExchange(feds, mode="ordered")


def _round(engines, feds, x, rnd, failed=(), late=(), results=None):
    for c, (e, fed) in enumerate(zip(engines, feds)):
        if results is not None:
            e.flat16.copy_(results[c][0])
            e.flat32.copy_(results[c][1])
        else:
            _train(e, fed, c, rnd)
        fed.pack(failed=c in failed)
    x.start()
    x.finish(list(late))
    for fed in feds:
        fed.unpack()
    return x.n_valid()


@pytest.mark.parametrize("opt", OPTS)
def test_all_invalid_round_keeps_the_state(opt):
    engines, feds, server, x = _local_group(opt, 2)
    rp = Replay(opt)
    assert _round(engines, feds, x, 0) == 2
    rp.round([0, 1], 0)
    before = _state(engines[0], feds[0], server)
    _assert_state(before, rp.state(), "round 0")
    assert _round(engines, feds, x, 1, failed=(0, 1)) == 0
    for e, fed in zip(engines, feds):  # back at the previous global copy; x, m, v keep their bits
        _assert_state(_state(e, fed, server), before, "the skipped round")
    assert _round(engines, feds, x, 2) == 2
    rp.round([0, 1], 2)  # the restatement that skipped that round
    for e, fed in zip(engines, feds):
        _assert_state(_state(e, fed, server), rp.state(), "round 2")


@pytest.mark.parametrize("opt,weights", [("fedavgm", None), ("fedyogi", (3, 1, 2))])
def test_late_failure_steps_once_on_the_re_exchanged_sum(opt, weights):
    engines, feds, server, x = _local_group(opt, 3, weights=weights)
    before = FedOptHostKernels.steps
    assert _round(engines, feds, x, 0, late=(0,)) == 2
    assert FedOptHostKernels.steps - before == 1
    rp = Replay(opt, weights=weights)
    rp.round([1, 2], 0)
    every = Replay(opt, weights=weights)
    every.round([0, 1, 2], 0)
    assert not torch.equal(rp.m, every.m)
    for e, fed in zip(engines, feds):
        _assert_state(_state(e, fed, server), rp.state(), opt)


@pytest.mark.parametrize("opt", OPTS)
def test_exact_identities(opt):
    # eta = 0: the delivered weights stay at the previous global copy (here fp16 values, so fp16(x) is x), m moves
    hp = dict(HP, lr=0.0)
    engines, feds, server, x = _local_group(opt, 2, hp=hp)
    for e, fed in zip(engines, feds):
        e.flat32.copy_(e.flat32.half().float())
        fed.snapshot()
    g16, g32 = feds[0].global16.clone(), feds[0].global32.clone()
    x0 = server.x.clone()
    assert torch.equal(x0, torch.cat([g16.float(), g32])) and not server.m.any()
    assert _round(engines, feds, x, 0) == 2
    for e, fed in zip(engines, feds):
        assert torch.equal(e.flat16, g16) and torch.equal(e.flat32, g32)
        assert torch.equal(fed.global16, g16) and torch.equal(fed.global32, g32)
    assert torch.equal(server.x, x0) and (server.m != 0).float().mean().item() > 0.9
    # two clients that return exactly the global weights: (g + g) / 2 is g, Delta = 0, x stays and m = 0
    engines, feds, server, x = _local_group(opt, 2)
    x0 = server.x.clone()
    same = [(e.flat16.clone(), e.flat32.clone()) for e in engines]
    assert _round(engines, feds, x, 0, results=same) == 2
    assert torch.equal(server.x, x0) and not server.m.any()
    if server.v is not None and opt != "fedadam":
        assert torch.equal(server.v, torch.full_like(x0, float(_f(HP["tau"]) * _f(HP["tau"]))))


# ----------------------------------------------------------------------------- the state and the config

def test_server_optimizer_state_dict():
    from federated_multi_modal_amd.federated import FedAvgBucket, ServerOptimizer
    e = _engine()
    sv = ServerOptimizer("fedadam", e, **HP)
    tau2 = float(_f(HP["tau"]) * _f(HP["tau"]))
    assert torch.equal(sv.x, torch.cat([e.flat16.float(), e.flat32])) and not sv.m.any()
    assert torch.equal(sv.v, torch.full_like(sv.x, tau2))
    assert ServerOptimizer("fedavgm", e).v is None
    sv.m.fill_(2.0)
    sd = sv.state_dict()
    assert sd["name"] == "fedadam" and (sd["n16"], sd["n32"]) == (N16, N32) and sd["hyper"] == HP
    assert all(sd[k].device.type == "cpu" and sd[k].dtype == torch.float32 for k in ("x", "m", "v"))
    other = ServerOptimizer("fedadam", e, **HP)
    other.load_state_dict(sd)
    assert torch.equal(other.m, sv.m) and torch.equal(other.x, sv.x) and torch.equal(other.v, sv.v)
    with pytest.raises(ValueError):
        ServerOptimizer("fedyogi", e, **HP).load_state_dict(sd)        # another optimizer
    with pytest.raises(ValueError):
        ServerOptimizer("fedadam", FakeEngine(0, n16=N16, n32=N32 + 1), **HP).load_state_dict(sd)  # other sizes
    with pytest.raises(ValueError):
        FedAvgBucket(FakeEngine(0, n16=N16, n32=N32 + 1), kernels=FedOptHostKernels, server=sv)
    # reset_from: back to the bucket's global copy
    fed = FedAvgBucket(e, kernels=FedOptHostKernels, server=sv)
    sv.x.add_(1.0)
    fed.snapshot()
    assert torch.equal(sv.x, torch.cat([e.flat16.float(), e.flat32])) and not sv.m.any()
    for bad in (dict(name="fedsgd"), dict(lr=-1.0), dict(lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.1),
                dict(tau=0.0)):
        kw = dict(HP, **{k: v for k, v in bad.items() if k != "name"})
        with pytest.raises(ValueError):
            ServerOptimizer(bad.get("name", "fedadam"), e, **kw)


def test_config_keys_and_their_defaults():
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    cfg = get_cfg_default()
    extend_cfg(cfg)
    assert cfg.FED.SERVER_OPT == "none"
    assert (cfg.FED.SERVER_LR, cfg.FED.SERVER_MOMENTUM, cfg.FED.SERVER_BETA2, cfg.FED.SERVER_TAU) == (1.0, 0.9, 0.99,
                                                                                                    1e-3)
    cfg.merge_from_list(["FED.SERVER_OPT", "fedyogi", "FED.SERVER_LR", 1, "FED.SERVER_TAU", "1e-2"])
    assert cfg.FED.SERVER_OPT == "fedyogi" and cfg.FED.SERVER_LR == 1.0 and cfg.FED.SERVER_TAU == 1e-2


def test_trainer_validates_the_server_keys():
    """MaPLeFederated._server_opt_cfg (what build_model calls first): each bad value raises ValueError naming its
    key."""
    from federated_multi_modal_amd.trainers import MaPLeFederated
    tr = MaPLeFederated.__new__(MaPLeFederated)
    tr.rank = 1
    good = {"SERVER_OPT": "fedadam", "SERVER_LR": 0.5, "SERVER_MOMENTUM": 0.9, "SERVER_BETA2": 0.99,
            "SERVER_TAU": 1e-3}
    name, hp = tr._server_opt_cfg(lambda k, d: good.get(k, d))
    assert name == "fedadam" and hp["FED.SERVER_LR"] == 0.5
    assert tr._server_opt_cfg(lambda k, d: d)[0] == "none"
    for key, val in (("SERVER_OPT", "fedsgd"), ("SERVER_MOMENTUM", 1.0), ("SERVER_MOMENTUM", -0.1),
                     ("SERVER_BETA2", 1.5), ("SERVER_LR", -1.0), ("SERVER_LR", float("inf")),
                     ("SERVER_LR", float("nan")), ("SERVER_TAU", 0.0), ("SERVER_TAU", -1e-3)):
        bad = dict(good, **{key: val})
        with pytest.raises(ValueError, match="FED." + key):
            tr._server_opt_cfg(lambda k, d, bad=bad: bad.get(k, d))
