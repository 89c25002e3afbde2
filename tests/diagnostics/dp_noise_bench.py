"""Diagnostic (GPU box): the DP-FedAvg kernels at the c4 trainable size (J = 9: 13 856 770 floats in the summed bucket),
timed with HIP events, each alternated in the same process with a yardstick that is not the code under test: torch's
in-place buf.add_(c) over the same buffer -- the noise kernel's bytes (one read, one write per float) and no
arithmetic.  10 warm-up rounds, medians of 40.  Not a gate: the kernels run once per round, beside seconds of training.

    python dp_noise_bench.py [out_file]
"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from federated_multi_modal_amd import ops  # noqa: E402

N = 13_856_770
WARMUP, REPS = 10, 40


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
    buf = torch.zeros(N, device=dev)
    # the scale kernels read the weights and the global copy: half of the trainables' floats in each flat buffer
    n16 = n32 = N // 2
    g16, g32 = torch.randn(n16, generator=g).half().to(dev), torch.randn(n32, generator=g).to(dev)
    p16 = (g16.float() + 1e-2 * torch.randn(n16, generator=g).to(dev)).half()
    p32 = g32 + 1e-2 * torch.randn(n32, generator=g).to(dev)
    ws, out = torch.zeros(ops.dp_update_ws_floats(n16, n32), device=dev), torch.zeros(3, device=dev)
    runs = {"yardstick add_": lambda: buf.add_(1e-3),
            "dp_add_noise": lambda: ops.dp_add_noise(buf, 0, 1234, 1, 1e-3),
            "dp_update_scale": lambda: ops.dp_update_scale(p16, g16, p32, g32, 1.0, ws, out)}
    times = {k: [] for k in runs}
    for it in range(WARMUP + REPS):
        for k, fn in runs.items():  # alternated: every kernel sees the same clocks and the same neighbours
            us = timed(fn)
            if it >= WARMUP:
                times[k].append(us)
        buf.zero_()
    nbytes = {"yardstick add_": 8.0 * N, "dp_add_noise": 8.0 * N, "dp_update_scale": 2.0 * (2 * n16 + 4 * n32)}
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{torch.cuda.get_device_name(0)}; {N} floats; {WARMUP} warm-up rounds, medians of {REPS}, alternated",
             f"{'kernel':18s} {'median us':>10s} {'min us':>9s} {'max us':>9s} {'GB/s':>8s} {'x yardstick':>12s}"]
    for k in runs:
        lines.append(f"{k:18s} {med[k]:10.1f} {min(times[k]):9.1f} {max(times[k]):9.1f} "
                     f"{nbytes[k] / med[k] / 1e3:8.1f} {med[k] / med['yardstick add_']:12.2f}")
    lines.append(f"dp_add_noise: {med['dp_add_noise'] * 1e3 / N:.4f} ns per float")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_file:
        Path(out_file).parent.mkdir(parents=True, exist_ok=True)
        Path(out_file).write_text(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
