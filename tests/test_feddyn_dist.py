"""CPU tier: FedDyn (FED.DYN_ALPHA; Acar, Zhao, Matas Navarro, Mattina, Whatmough, Saligrama: "Federated Learning Based
on Dynamic Regularization", ICLR 2021) through federated.FedDynState and the collective protocol of
federated_multi_modal_amd/federated.py on gloo ranks, with a host restatement of mf_feddyn_step / mf_feddyn_deliver in
the kernels' place (the GPU tier, tests/test_feddyn_gpu.py, checks the kernels against the same restatement bit for
bit).

host_round_end is the restatement: torch fp32 on the CPU, one torch op per rounding point of the kernel, alpha as an
fp32 tensor, frac = votes / N and af = alpha * frac formed in fp32.  Everything else here compares with it bit for bit;
test_restatement_against_the_paper ties it to Algorithm 1 and test_spot_values to numbers worked by hand."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_fedavg_dist import FakeEngine, HostKernels, _init, _spawn
from test_fedopt_dist import N16, N32, _engine, _f, local_result

ALPHA = 0.1  # not an fp32 value: the rounding of alpha itself is part of what is compared


def host_round_end(total, votes, num_clients, alpha, w, q, h, lam, take, step):
    """FedDyn's round end for one client on fp32 CPU tensors.  total: the summed bucket's n values; votes: its vote
    count (a 0-dim fp32 tensor, > 0); w, q: the client's local weights and the round's starting weights as fp32;
    take: the client took part (its flag is 0); step: h is stepped (mf_feddyn_step) or only read (mf_feddyn_deliver).
    Returns (x, h, lam), x before its fp16 rounding."""
    a = _f(alpha)
    if take:
        lam = lam - a * (w - q)
    mean = total / votes
    if step:
        af = a * (votes / _f(num_clients))
        h = h - af * (mean - q)
    return mean - h / a, h, lam


class FedDynHostKernels(HostKernels):
    """The host kernels plus FedDyn's round end, with ops.feddyn_step's / ops.feddyn_deliver's signatures."""
    steps = 0     # per process: how many times h was stepped
    delivers = 0

    @staticmethod
    def _apply(bucket, alpha, num_clients, h, lam, flag, p16, p32, g16, g32, step):
        n16 = p16.numel()
        n = n16 + p32.numel()
        if float(bucket[n]) == 0:
            p16.copy_(g16)
            p32.copy_(g32)
            return
        w, q = torch.cat([p16.float(), p32]), torch.cat([g16.float(), g32])
        x, hn, ln = host_round_end(bucket[:n], bucket[n], num_clients, alpha, w, q, h, lam, int(flag.item()) == 0, step)
        h.copy_(hn)
        lam.copy_(ln)
        val = x.half()
        p16.copy_(val[:n16])
        p32.copy_(val[n16:].float())
        g16.copy_(p16)
        g32.copy_(p32)

    @classmethod
    def feddyn_step(cls, bucket, alpha, num_clients, h, lam, flag, p16, p32, g16, g32):
        cls.steps += 1
        cls._apply(bucket, alpha, num_clients, h, lam, flag, p16, p32, g16, g32, True)

    @classmethod
    def feddyn_deliver(cls, bucket, alpha, h, lam, flag, p16, p32, g16, g32):
        cls.delivers += 1
        cls._apply(bucket, alpha, 1, h.clone(), lam, flag, p16, p32, g16, g32, False)


class Replay:
    """The single-process restatement of the rounds over all N clients: the valid clients' results summed in client
    order, each valid client's lam updated, h stepped once per round with a vote, fp16(x) delivered to everyone."""

    def __init__(self, num_clients, alpha=ALPHA, n16=N16, n32=N32):
        e = FakeEngine(0, n16=n16, n32=n32)
        self.N, self.alpha, self.n16 = num_clients, alpha, n16
        self.g16, self.g32 = e.flat16.clone(), e.flat32.clone()
        self.h = torch.zeros(n16 + n32)
        self.lam = [torch.zeros(n16 + n32) for _ in range(num_clients)]

    def round(self, valid, rnd, results=None):
        """valid: the clients that took part, in client order.  results: {client: (p16, p32)} instead of
        local_result."""
        if not valid:
            return
        ws = {}
        for c in valid:
            p16, p32 = results[c] if results is not None else local_result(c, rnd, self.g16, self.g32)
            ws[c] = torch.cat([p16.float(), p32])
        acc = votes = None
        for c in valid:
            acc = ws[c].clone() if acc is None else acc + ws[c]
            votes = _f(1.0) if votes is None else votes + _f(1.0)
        q = torch.cat([self.g16.float(), self.g32])
        x = None
        for i, c in enumerate(valid):
            x, h, self.lam[c] = host_round_end(acc, votes, self.N, self.alpha, ws[c], q, self.h, self.lam[c], True,
                                               i == 0)
            if i == 0:
                self.h = h
        val = x.half()
        self.g16, self.g32 = val[:self.n16].clone(), val[self.n16:].float()


def _bucket(e, dyn=None, num_clients=1, mode="ordered", alpha=ALPHA):
    from federated_multi_modal_amd.federated import FedAvgBucket, FedDynState
    if dyn is None:
        dyn = FedDynState(alpha, e, num_clients)
    return FedAvgBucket(e, kernels=FedDynHostKernels, mode=mode, dyn=dyn), dyn


def _train(e, fed, client, rnd):
    p16, p32 = local_result(client, rnd, fed.global16, fed.global32)
    e.flat16.copy_(p16)
    e.flat32.copy_(p32)


def _state(e, fed, dyn):
    return tuple(t.clone() for t in (e.flat16, e.flat32, fed.global16, fed.global32, dyn.h, fed.lam))


NAMES = ("p16", "p32", "g16", "g32", "h", "lam")


def _assert_state(got, rp, client, what=""):
    want = (rp.g16, rp.g32, rp.g16, rp.g32, rp.h, rp.lam[client])
    for k, a, b in zip(NAMES, got, want):
        assert torch.equal(a, b), f"{what} {k}"


# ----------------------------------------------------------------------------- 1. the exchange protocol

def _rounds_worker(rank, world, port, mode, out):
    _init(rank, world, port)
    e = _engine()
    fed, dyn = _bucket(e, num_clients=world, mode=mode)
    for rnd in range(2):
        _train(e, fed, rank, rnd)
        assert fed.run() == world
    out[rank] = _state(e, fed, dyn)
    dist.destroy_process_group()


@pytest.mark.parametrize("world,mode", [(2, "ordered"), (3, "ordered"), (2, "allreduce")])
def test_exchange_two_rounds_bit_exact(world, mode):
    """One client per rank, two consecutive rounds: the weights, the global copy, h and the client's lam of every rank
    equal the single-process replay bit for bit (a sum of two values does not depend on its order, so "allreduce" at
    world 2 does too)."""
    res = _spawn(_rounds_worker, world, mode)
    rp, first = Replay(world), Replay(world)
    first.round(list(range(world)), 0)
    for rnd in range(2):
        rp.round(list(range(world)), rnd)
    assert not torch.equal(rp.h, first.h) and not torch.equal(rp.lam[0], first.lam[0])  # the second round did something
    assert rp.h.any() and all(lam.any() for lam in rp.lam)
    for r in range(world):
        _assert_state(res[r], rp, r, f"rank {r}")
        assert torch.equal(res[r][4], res[0][4]), f"h of rank {r} vs rank 0"


def _group_worker(rank, world, port, per_rank, out):
    _init(rank, world, port)
    from federated_multi_modal_amd.federated import FedAvgExchange
    ids = list(range(rank * per_rank, (rank + 1) * per_rank))
    engines = [_engine() for _ in ids]
    dyn, feds = None, []
    for e in engines:
        fed, dyn = _bucket(e, dyn, world * per_rank)
        feds.append(fed)
    x = FedAvgExchange(feds, mode="ordered")
    for c, e, fed in zip(ids, engines, feds):
        _train(e, fed, c, 0)
        fed.pack()
    x.start()
    x.finish([])
    for fed in feds:
        fed.unpack()
    out[rank] = ([_state(e, f, dyn) for e, f in zip(engines, feds)], FedDynHostKernels.steps,
                 FedDynHostKernels.delivers, x.n_valid())
    dist.destroy_process_group()


def test_two_clients_per_rank_one_step_one_deliver():
    res = _spawn(_group_worker, 2, 2)
    rp = Replay(4)
    rp.round([0, 1, 2, 3], 0)
    for r in range(2):
        states, steps, delivers, n_valid = res[r]
        assert (steps, delivers, n_valid) == (1, 1, 4)
        for j, st in enumerate(states):  # both local clients: the same delivered bits, each its own updated lam
            _assert_state(st, rp, 2 * r + j, f"rank {r} client {j}")
        assert states[0][5].any() and states[1][5].any() and not torch.equal(states[0][5], states[1][5])


def _local_group(n, alpha=ALPHA, make_engine=_engine):
    from federated_multi_modal_amd.federated import FedAvgExchange
    engines = [make_engine() for _ in range(n)]
    dyn, feds = None, []
    for e in engines:
        fed, dyn = _bucket(e, dyn, n, alpha=alpha)
        feds.append(fed)
    return engines, feds, dyn, FedAvgExchange(feds, mode="ordered")


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


def test_all_invalid_round_keeps_h_and_every_lam():
    engines, feds, dyn, x = _local_group(2)
    rp = Replay(2)
    assert _round(engines, feds, x, 0) == 2
    rp.round([0, 1], 0)
    before = [_state(e, f, dyn) for e, f in zip(engines, feds)]
    for c, st in enumerate(before):
        _assert_state(st, rp, c, "round 0")
    assert _round(engines, feds, x, 1, failed=(0, 1)) == 0
    for c, (e, fed) in enumerate(zip(engines, feds)):  # back at the global copy; h and lam keep their bits
        for k, a, b in zip(NAMES, _state(e, fed, dyn), before[c]):
            assert torch.equal(a, b), k
    assert _round(engines, feds, x, 2) == 2
    rp.round([0, 1], 2)  # the replay that skipped that round
    for c, (e, fed) in enumerate(zip(engines, feds)):
        _assert_state(_state(e, fed, dyn), rp, c, "round 2")


def test_an_invalid_client_keeps_its_lam_and_reaches_h_through_frac():
    engines, feds, dyn, x = _local_group(3)
    rp = Replay(3)
    assert _round(engines, feds, x, 0) == 3
    rp.round([0, 1, 2], 0)
    lam1 = feds[1].lam.clone()
    results = [local_result(c, 1, feds[0].global16, feds[0].global32) for c in range(3)]
    results[1][1][5] = float("inf")  # the validity scan sets client 1's flag
    assert _round(engines, feds, x, 1, results=results) == 2
    rp.round([0, 2], 1, results=dict(enumerate(results)))
    assert torch.equal(feds[1].lam, lam1)
    for c, (e, fed) in enumerate(zip(engines, feds)):
        _assert_state(_state(e, fed, dyn), rp, c, f"client {c}")


def test_late_failure_steps_once_on_the_re_exchanged_sum():
    engines, feds, dyn, x = _local_group(3)
    before = FedDynHostKernels.steps
    assert _round(engines, feds, x, 0, late=(0,)) == 2
    assert FedDynHostKernels.steps - before == 1
    rp, every = Replay(3), Replay(3)
    rp.round([1, 2], 0)  # frac = 2 / 3
    every.round([0, 1, 2], 0)
    assert not torch.equal(rp.h, every.h)
    assert not feds[0].lam.any()  # the failed client's lam keeps its bits
    for c, (e, fed) in enumerate(zip(engines, feds)):
        _assert_state(_state(e, fed, dyn), rp, c, f"client {c}")
    assert torch.equal(feds[1].lam, every.lam[1])  # the others updated once, from their own weights


# ----------------------------------------------------------------------------- 2. h is the mean of the lam_k

def test_h_is_the_mean_of_the_corrections():
    """With every client valid h and (1/N) sum_k lam_k are the same number in exact arithmetic: alpha * (mean_k w_k - q)
    is mean_k alpha * (w_k - q).  In fp32 they differ by the roundings, u = 2^-24 each, per element, with
    W = max |w_k|, D = max |w_k - q| over the clients and rounds and |lam_k|, |h| <= R alpha D after R rounds:
      lam_k per round: w - q (<= u D), times alpha (<= u alpha D, on top of alpha u D carried over), the difference
        (<= u |lam_k|): 2 u alpha D + u r alpha D in round r, and their mean over k is no larger;
      h per round: the sum of N values (N - 1 additions of partial sums <= N W: (N - 1) u N W, divided by N), the
        division (u W), mean - q (u D), times af = alpha exactly (votes == N: frac is 1) (u alpha D), the difference
        (u |h|): alpha u (N W + 2 D) + u r alpha D.
    Summed over r = 1 .. R: |h - mean lam| <= R alpha u (N W + 4 D) + u alpha D R (R + 1); the second-order terms are
    2^-24 of that and covered by the factor 1.001.  The mean of the fp32 lam_k is formed in fp64 (exact for three
    fp32 values up to the final division's 2^-53)."""
    N, R = 3, 4
    engines, feds, dyn, x = _local_group(N)
    n = N16 + N32
    W, D = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for rnd in range(R):
        q = torch.cat([feds[0].global16.float(), feds[0].global32]).double()
        results = [local_result(c, rnd, feds[0].global16, feds[0].global32) for c in range(N)]
        for p16, p32 in results:
            w = torch.cat([p16.float(), p32]).double()
            W, D = torch.maximum(W, w.abs()), torch.maximum(D, (w - q).abs())
        assert _round(engines, feds, x, rnd, results=results) == N
    u, a = 2.0 ** -24, float(_f(ALPHA))
    bound = 1.001 * (R * a * u * (N * W + 4 * D) + u * a * D * R * (R + 1))
    mean = sum(f.lam.double() for f in feds) / N
    err = (dyn.h.double() - mean).abs()
    print(f"|h - mean lam|: max {err.max().item():.3e}, largest share of the bound {(err / bound).max().item():.3f}")
    assert dyn.h.abs().max().item() > 1e-3  # the corrections are far above the bound
    assert (err <= bound).all()


# ----------------------------------------------------------------------------- 3. the fixed point

def test_fixed_point_is_the_global_optimum():
    """Four clients with losses 0.5 a_k (theta - c_k)^2, a_k ~ U(0.5, 4), c_k ~ N(0, 1), 4096 coordinates.  Each round's
    local training is the exact minimiser of the FedDyn objective 0.5 a_k (theta - c_k)^2 - lam_k theta +
    0.5 alpha (theta - g)^2, theta_k = (a_k c_k + lam_k + alpha g) / (a_k + alpha); alpha = 1, 20 rounds through
    FedAvgBucket with its fp16 delivery.  Plain FedAvg of the clients' exact minimisers sits at mean c_k, away from the
    optimum sum a_k c_k / sum a_k; FedDyn's global weights end within 1 / 50 of that distance (the largest coordinate's
    and the Euclidean one alike)."""
    K, n, alpha = 4, 4096, 1.0
    gen = torch.Generator().manual_seed(3)
    a = 0.5 + 3.5 * torch.rand(K, n, generator=gen)
    c = torch.randn(K, n, generator=gen)
    opt = (a * c).sum(0) / a.sum(0)
    fedavg = c.mean(0)

    def start():
        e = FakeEngine(0, n16=0, n32=n)
        e.flat32.zero_()
        return e

    engines, feds, dyn, x = _local_group(K, alpha=alpha, make_engine=start)
    for rnd in range(20):
        g = feds[0].global32
        results = [(torch.empty(0, dtype=torch.float16), (a[k] * c[k] + feds[k].lam + alpha * g) / (a[k] + alpha))
                   for k in range(K)]
        assert _round(engines, feds, x, rnd, results=results) == K
    got = feds[0].global32
    for norm in (lambda t: t.abs().max().item(), lambda t: t.norm().item()):
        d_dyn, d_avg = norm(got - opt), norm(fedavg - opt)
        print(f"distance to the optimum: FedDyn {d_dyn:.3e}, plain FedAvg's fixed point {d_avg:.3e}")
        assert d_dyn <= d_avg / 50


# ----------------------------------------------------------------------------- 4. the restatement against the paper

def paper_algorithm_1(alpha, num_clients, rounds):
    """Algorithm 1 of Acar et al. in numpy fp64, written from the paper, for given local results.  rounds: per round
    (theta_prev, {k: theta_k}) -- the server model the round started from and the participating devices' local models.
      device k in P_t:   grad_k = grad_k - alpha (theta_k - theta_prev)          (devices not in P_t keep theirs)
      server:            h = h - alpha (1 / m) sum_{k in P_t} (theta_k - theta_prev)
                         theta = (1 / |P_t|) sum_{k in P_t} theta_k - h / alpha
    Returns per round (theta, h, [grad_k]).  alpha is the fp32 value the kernel is handed."""
    alpha = np.float64(np.float32(alpha))
    m = num_clients
    n = next(iter(rounds[0][1].values())).shape[0]
    h, grads, out = np.zeros(n), [np.zeros(n) for _ in range(m)], []
    for theta_prev, thetas in rounds:
        for k, th in thetas.items():
            grads[k] = grads[k] - alpha * (th - theta_prev)
        h = h - alpha * (1.0 / m) * np.sum([th - theta_prev for th in thetas.values()], axis=0)
        theta = np.sum(list(thetas.values()), axis=0) / len(thetas) - h / alpha
        out.append((theta, h.copy(), [g.copy() for g in grads]))
    return out


# the largest deviation of the fp32 restatement from the fp64 statement over the three rounds, measured on an x86-64
# host on the inputs below: of x relative to s, of h and lam relative to alpha * s, s = the element's largest |w| over
# the clients and rounds.  The gate is twice that.
PAPER_MEASURED = {"x": 2.65e-7, "h": 2.37e-7, "lam": 2.21e-7}


def test_restatement_against_the_paper():
    """host_round_end over three rounds, three clients, client 1 absent in round 2, against paper_algorithm_1: 4096
    values spread over twelve binades, alpha = 0.1, rounds whose updates differ in size by 2^8.  Both sides are handed
    the same round-start weights (the fp16 values the restatement delivered), so what is compared is the arithmetic of
    the round's end.  Measured deviation, max over elements and rounds (PAPER_MEASURED):
        x 2.65e-7 of s,  h 2.37e-7 and lam 2.21e-7 of alpha * s,  s = the element's largest |w|
    and the gate is twice the measured value.  All three are a few units of u = 2^-24 = 6e-8:
    the sum of three weights, the division and the differences each round to within u of a value of the size of s,
    and h / alpha hands h's error back to x at the scale it had before alpha was taken off."""
    N, n = 3, 4096
    gen = torch.Generator().manual_seed(11)
    q = (torch.randn(n, generator=gen) * torch.exp2(torch.randint(-6, 6, (n,), generator=gen).float())).half().float()
    h, lam = torch.zeros(n), [torch.zeros(n) for _ in range(N)]
    fp64_rounds, got, s = [], [], torch.zeros(n)
    for scale, valid in ((2.0 ** -3, (0, 1, 2)), (2.0 ** -8, (0, 2)), (1.0, (0, 1, 2))):
        ws = {k: q * (1.0 + scale * torch.randn(n, generator=gen)) + scale * 1e-2 * torch.randn(n, generator=gen)
              for k in valid}
        s = torch.maximum(s, torch.stack(list(ws.values())).abs().max(0).values)
        fp64_rounds.append((q.double().numpy(), {k: w.double().numpy() for k, w in ws.items()}))
        acc = votes = None
        for k in valid:
            acc = ws[k].clone() if acc is None else acc + ws[k]
            votes = _f(1.0) if votes is None else votes + _f(1.0)
        for i, k in enumerate(valid):
            x, hn, lam[k] = host_round_end(acc, votes, N, ALPHA, ws[k], q, h, lam[k], True, i == 0)
            if i == 0:
                h = hn
        got.append((x.clone(), h.clone(), [t.clone() for t in lam]))
        q = x.half().float()
    ref = paper_algorithm_1(ALPHA, N, fp64_rounds)
    s64, a = s.double().numpy(), float(_f(ALPHA))
    dev = {"x": 0.0, "h": 0.0, "lam": 0.0}
    for (x32, h32, l32), (x64, h64, l64) in zip(got, ref):
        dev["x"] = max(dev["x"], float(np.max(np.abs(x32.double().numpy() - x64) / s64)))
        dev["h"] = max(dev["h"], float(np.max(np.abs(h32.double().numpy() - h64) / (a * s64))))
        for t32, t64 in zip(l32, l64):
            dev["lam"] = max(dev["lam"], float(np.max(np.abs(t32.double().numpy() - t64) / (a * s64))))
    for k, v in dev.items():
        print(f"fp32 restatement vs fp64 Algorithm 1, {k}: max deviation {v:.3e} (gate {2 * PAPER_MEASURED[k]:.3e})")
    # client 1 sat round 2 out: its correction kept its bits there, and h is not the all-clients' step
    assert torch.equal(got[1][2][1], got[0][2][1]) and np.array_equal(ref[1][2][1], ref[0][2][1])
    assert np.abs(ref[2][1]).max() > 0
    for k, v in dev.items():
        assert v <= 2 * PAPER_MEASURED[k], k


def test_spot_values():
    """One element through two rounds, worked by hand on numbers fp32 holds exactly (every intermediate is exact): what
    catches a wrong formula that the kernel and the restatement would share.  alpha = 0.5, N = 2.
      round 1, q = 1, w = (3, 5): lam = (0 - 0.5 * 2, 0 - 0.5 * 4) = (-1, -2); mean = 8 / 2 = 4; af = 0.5 * (2 / 2);
        h = 0 - 0.5 * (4 - 1) = -1.5 (the mean of the lam); x = 4 - (-1.5 / 0.5) = 7
      round 2, q = 7, client 0 alone with w = 6: lam_0 = -1 - 0.5 * (6 - 7) = -0.5, lam_1 stays -2; mean = 6;
        af = 0.5 * (1 / 2) = 0.25; h = -1.5 - 0.25 * (6 - 7) = -1.25 (again their mean); x = 6 - (-1.25 / 0.5) = 8.5"""
    one = lambda v: torch.tensor([float(v)])  # noqa: E731
    x, h, l0 = host_round_end(one(8), _f(2), 2, 0.5, one(3), one(1), one(0), one(0), True, True)
    assert (x.item(), h.item(), l0.item()) == (7.0, -1.5, -1.0)
    x1, h1, l1 = host_round_end(one(8), _f(2), 2, 0.5, one(5), one(1), h, one(0), True, False)
    assert (x1.item(), h1.item(), l1.item()) == (7.0, -1.5, -2.0)
    x, h, l0 = host_round_end(one(6), _f(1), 2, 0.5, one(6), one(7), h, l0, True, True)
    assert (x.item(), h.item(), l0.item()) == (8.5, -1.25, -0.5)
    # the absent client: the same delivered value, its lam untouched
    x1, h1, l1 = host_round_end(one(6), _f(1), 2, 0.5, one(float("nan")), one(7), h, l1, False, False)
    assert (x1.item(), h1.item(), l1.item()) == (8.5, -1.25, -2.0)
    assert h.item() == (l0.item() + l1.item()) / 2


# ----------------------------------------------------------------------------- 5. the state and the config

def test_state_dicts():
    from federated_multi_modal_amd.federated import FedAvgBucket, FedDynState, ServerOptimizer
    e = _engine()
    dyn = FedDynState(ALPHA, e, 3)
    assert dyn.h.dtype == torch.float32 and dyn.h.numel() == N16 + N32 and not dyn.h.any() and not dyn.pending
    fed = FedAvgBucket(e, kernels=FedDynHostKernels, dyn=dyn)
    assert fed.lam.dtype == torch.float32 and fed.lam.numel() == N16 + N32 and not fed.lam.any()
    dyn.h.fill_(2.0)
    fed.lam.fill_(3.0)
    sd = dyn.state_dict()
    assert (sd["alpha"], sd["num_clients"], sd["n16"], sd["n32"]) == (ALPHA, 3, N16, N32)
    assert sd["h"].device.type == "cpu" and sd["h"].dtype == torch.float32
    other = FedDynState(ALPHA, e, 3)
    other.load_state_dict(sd)
    assert torch.equal(other.h, dyn.h)
    bigger = FakeEngine(0, n16=N16, n32=N32 + 1)
    with pytest.raises(ValueError):
        FedDynState(ALPHA, bigger, 3).load_state_dict(sd)   # other sizes
    with pytest.raises(ValueError):
        other.load_state_dict(dict(sd, h=sd["h"].double()))
    with pytest.raises(ValueError):
        FedAvgBucket(bigger, kernels=FedDynHostKernels, dyn=dyn)
    bsd = fed.state_dict()
    assert bsd["residual"] is None and torch.equal(bsd["lam"], fed.lam) and bsd["lam"].device.type == "cpu"
    fed2 = FedAvgBucket(e, kernels=FedDynHostKernels, dyn=dyn)
    fed2.load_state_dict(bsd)
    assert torch.equal(fed2.lam, fed.lam)
    fed2.load_state_dict({"residual": None})  # no lam: the correction restarts
    assert not fed2.lam.any()
    with pytest.raises(ValueError):
        fed2.load_state_dict({"residual": None, "lam": bsd["lam"][:-1]})
    with pytest.raises(ValueError):
        fed2.load_state_dict({"residual": None, "lam": bsd["lam"].half()})
    plain = FedAvgBucket(e, kernels=FedDynHostKernels)
    assert plain.lam is None and plain.state_dict() == {"residual": None}
    with pytest.raises(ValueError):
        plain.load_state_dict(bsd)  # a lam for a bucket without FedDyn
    # snapshot: weights from outside the round loop restart the corrections
    fed.snapshot()
    assert not fed.lam.any() and not dyn.h.any()
    for bad in ((0.0, 3), (-0.1, 3), (float("nan"), 3), (float("inf"), 3), (ALPHA, 0), (ALPHA, 2.0)):
        with pytest.raises(ValueError):
            FedDynState(bad[0], e, bad[1])
    # FedDyn needs the clients' own weights in a plain mean
    for kw in (dict(weight=2.0), dict(robust="median"), dict(dp_clip=1.0), dict(compress="int8"),
               dict(server=ServerOptimizer("fedavgm", e))):
        with pytest.raises(ValueError, match="plain mean"):
            FedAvgBucket(e, kernels=FedDynHostKernels, dyn=dyn, **kw)
    FedAvgBucket(e, kernels=FedDynHostKernels, dyn=dyn, mode="allreduce")  # both exchange modes are allowed


def test_config_key_and_its_default():
    from federated_multi_modal_amd.config import extend_cfg, get_cfg_default
    cfg = get_cfg_default()
    extend_cfg(cfg)
    assert cfg.FED.DYN_ALPHA == 0.0
    cfg.merge_from_list(["FED.DYN_ALPHA", 0.1])
    assert cfg.FED.DYN_ALPHA == 0.1


def test_trainer_validates_the_key():
    """MaPLeFederated._dyn_cfg (what build_model calls once the other options are read): a bad alpha and each rejected
    combination raise ValueError naming the key."""
    from federated_multi_modal_amd.trainers import MaPLeFederated
    tr = MaPLeFederated.__new__(MaPLeFederated)
    tr.rank = 1
    tr.client_weights = None
    tr.dp = {"clip": None}
    tr.compress = {"compress": None}
    cfg = lambda **kw: (lambda k, d: kw.get(k, d))  # noqa: E731
    assert tr._dyn_cfg(cfg(), 0.0, "none", None) == 0.0
    assert tr._dyn_cfg(cfg(DYN_ALPHA=0.1), 0.0, "none", None) == 0.1
    assert tr._dyn_cfg(cfg(DYN_ALPHA=0), 0.5, "fedadam", "median") == 0.0  # off: nothing to reject
    for bad in (-0.1, float("nan"), float("inf"), "0.1", True):
        with pytest.raises(ValueError, match="FED.DYN_ALPHA"):
            tr._dyn_cfg(cfg(DYN_ALPHA=bad), 0.0, "none", None)
    on = cfg(DYN_ALPHA=0.1)
    with pytest.raises(ValueError, match="FED.PROX_MU"):
        tr._dyn_cfg(on, 0.5, "none", None)
    with pytest.raises(ValueError, match="FED.SERVER_OPT"):
        tr._dyn_cfg(on, 0.0, "fedadam", None)
    with pytest.raises(ValueError, match="FED.ROBUST_AGG"):
        tr._dyn_cfg(on, 0.0, "none", "median")
    tr.client_weights = [3.0, 1.0]
    with pytest.raises(ValueError, match="FED.CLIENT_WEIGHTS"):
        tr._dyn_cfg(cfg(DYN_ALPHA=0.1, CLIENT_WEIGHTS="3,1"), 0.0, "none", None)
    tr.client_weights = None
    tr.dp = {"clip": 1.0}
    with pytest.raises(ValueError, match="FED.DP_CLIP"):
        tr._dyn_cfg(on, 0.0, "none", None)
    tr.dp = {"clip": None}
    tr.compress = {"compress": "int8"}
    with pytest.raises(ValueError, match="FED.COMPRESS"):
        tr._dyn_cfg(on, 0.0, "none", None)
