"""Diagnostic (GPU box): FedDyn's kernels at the c4 trainable size (n16 = 10 630 144 fp16 and n32 = 3 226 624 fp32
trainables), timed with HIP events around each call, each beside the kernels they stand next to: mf_feddyn_step and
mf_feddyn_deliver beside mf_fedavg_unpack on the same summed bucket, and the dynamic SGD launches (mf_sgd_dyn_step over
the fp16 and the fp32 buffer) beside the proximal and the plain ones.  All of them alternated in the same process, 10
warm-up rounds, medians of 40; bytes moved, TB/s and the fraction of the 8 TB/s HBM peak.  Not a gate: the round's end
runs once per client and round, beside seconds of training.

    python feddyn_bench.py [out_file]
"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from federated_multi_modal_amd import ops  # noqa: E402

N16, N32 = 10_630_144, 3_226_624
WARMUP, REPS = 10, 40
PEAK = 8.0e12
ALPHA, CLIENTS = 0.1, 4


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def main(out_file=None):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = N16 + N32
    g16, g32 = torch.randn(N16, generator=g).half().to(dev), torch.randn(N32, generator=g).to(dev)
    p16 = (g16.float() + 1e-2 * torch.randn(N16, generator=g).to(dev)).half()
    p32 = g32 + 1e-2 * torch.randn(N32, generator=g).to(dev)
    # the sum of CLIENTS clients near the global weights, and their votes
    bucket = torch.cat([p16.float(), p32, torch.ones(1, device=dev)]) * float(CLIENTS)
    h, lam = torch.zeros(n, device=dev), 1e-3 * torch.randn(n, generator=g).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    # the local step: gradients, momentum, a clip coefficient of 1, the momentum path
    gr16, gr32 = (1e-2 * torch.randn(N16, generator=g)).half().to(dev), (1e-2 * torch.randn(N32, generator=g)).to(dev)
    b16, b32 = torch.zeros_like(gr16), torch.zeros_like(gr32)
    coef = torch.tensor([1.0, 1.0, 1.0], device=dev)
    hyper5 = torch.tensor([1e-3, 0.9, 5e-4, 0.0, 0.0], device=dev)
    hyper6 = torch.tensor([1e-3, 0.9, 5e-4, 0.0, 0.0, ALPHA], device=dev)
    weights = 2 * N16 + 4 * N32

    def plain():
        ops.sgd_step(p16, gr16, b16, coef, hyper5)
        ops.sgd_step(p32, gr32, b32, coef, hyper5)

    def prox():
        ops.sgd_prox_step(p16, gr16, b16, g16, coef, hyper6)
        ops.sgd_prox_step(p32, gr32, b32, g32, coef, hyper6)

    def dyn():
        ops.sgd_dyn_step(p16, gr16, b16, g16, lam[:N16], coef, hyper6)
        ops.sgd_dyn_step(p32, gr32, b32, g32, lam[N16:], coef, hyper6)

    runs = {
        # bucket read; the weights and the global copy written
        "fedavg_unpack": (lambda: ops.fedavg_unpack(bucket, p16, p32, g16, g32), 4 * n + 2 * weights),
        # ... h and lam read and written, the weights and the global copy read too
        "feddyn_step": (lambda: ops.feddyn_step(bucket, ALPHA, CLIENTS, h, lam, flag, p16, p32, g16, g32),
                        4 * n + 16 * n + 4 * weights),
        # ... h only read
        "feddyn_deliver": (lambda: ops.feddyn_deliver(bucket, ALPHA, h, lam, flag, p16, p32, g16, g32),
                           4 * n + 12 * n + 4 * weights),
        # p, g, momentum read; g, momentum, p written -- the two launches of the fp16 and the fp32 buffer
        "sgd plain (2 launches)": (plain, 6 * weights),
        "sgd proximal": (prox, 7 * weights),
        "sgd dynamic": (dyn, 7 * weights + 4 * n),
    }
    times = {k: [] for k in runs}
    for it in range(WARMUP + REPS):
        for k, (fn, _) in runs.items():  # alternated: every kernel sees the same clocks and the same neighbours
            t = timed(fn)
            if it >= WARMUP:
                times[k].append(t)
    lines = [f"{torch.cuda.get_device_name(0)}; n16 = {N16}, n32 = {N32}; {WARMUP} warm-up rounds, medians of {REPS}, "
             "alternated",
             f"{'kernel':24s} {'MB':>7s} {'median us':>10s} {'min us':>8s} {'max us':>8s} {'TB/s':>6s} {'of peak':>8s}"]
    for k, (_, nb) in runs.items():
        med = statistics.median(times[k])
        lines.append(f"{k:24s} {nb / 1e6:7.1f} {med:10.1f} {min(times[k]):8.1f} {max(times[k]):8.1f} "
                     f"{nb / med / 1e6:6.2f} {nb / med * 1e6 / PEAK:8.2f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_file:
        Path(out_file).parent.mkdir(parents=True, exist_ok=True)
        Path(out_file).write_text(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
