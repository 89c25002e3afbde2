"""Diagnostic (GPU box): the uplink compression kernels at the c4 trainable size (J = 9: 13 856 770 coordinates, half of
them taken as fp16 and half as fp32 trainables), timed with HIP events, each alternated in the same process with a
yardstick that is not the code under test: a torch copy that moves the same number of bytes (half of them read, half
written).  10 warm-up rounds, medians of 40.  Not a gate: the kernels run once per client and round, beside seconds of
training.

    python compress_bench.py [out_file]
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
    n16 = n32 = N // 2
    g16, g32 = torch.randn(n16, generator=g).half().to(dev), torch.randn(n32, generator=g).to(dev)
    p16 = (g16.float() + 1e-2 * torch.randn(n16, generator=g).to(dev)).half()
    p32 = g32 + 1e-2 * torch.randn(n32, generator=g).to(dev)
    S = -(-(N + 1) // ops.COMPRESS_BLOCK) * ops.COMPRESS_BLOCK  # one destination rank
    chunk = ops.compress_chunk_bytes(S)
    image = torch.zeros(1, 1, chunk, dtype=torch.uint8, device=dev)
    e_in, e_out = 1e-4 * torch.randn(N, generator=g).to(dev), torch.zeros(N, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros(S, device=dev)
    weights = 2 * (2 * n16 + 4 * n32)  # the weights and the global copy, read
    nbytes = {"quantize nearest": weights + 8 * N + chunk, "quantize stochastic": weights + 8 * N + chunk,
              "quantize, no feedback": weights + chunk, "decode": chunk + weights // 2 + 4 * S}
    copies = {}
    for k, b in nbytes.items():
        src, dst = torch.zeros(b // 2, dtype=torch.uint8, device=dev), torch.zeros(b // 2, dtype=torch.uint8, device=dev)
        copies[k] = (lambda s=src, d=dst: d.copy_(s))

    def quantize(rounding, feedback=True):
        ops.compress_quantize(p16, p32, g16, g32, e_in if feedback else None, e_out if feedback else None, flag, None,
                              rounding, 1234, 1, 0, image, 0, S)

    runs = {"quantize nearest": lambda: quantize("nearest"), "quantize stochastic": lambda: quantize("stochastic"),
            "quantize, no feedback": lambda: quantize("stochastic", False),
            "decode": lambda: ops.compress_decode(image.view(-1), 1, chunk, S, 0, 0, g16, g32, "plain", out, S)}
    times = {k: [] for k in runs}
    yard = {k: [] for k in runs}
    for it in range(WARMUP + REPS):
        for k, fn in runs.items():  # alternated: every kernel sees the same clocks and the same neighbours
            a, b = timed(copies[k]), timed(fn)
            if it >= WARMUP:
                yard[k].append(a)
                times[k].append(b)
    lines = [f"{torch.cuda.get_device_name(0)}; {N} coordinates, S = {S}, chunk = {chunk} bytes; {WARMUP} warm-up rounds, "
             f"medians of {REPS}, alternated",
             f"{'kernel':24s} {'MB':>7s} {'median us':>10s} {'min us':>8s} {'max us':>8s} {'GB/s':>7s} "
             f"{'copy us':>8s} {'x copy':>7s}"]
    for k in runs:
        med, ymed = statistics.median(times[k]), statistics.median(yard[k])
        lines.append(f"{k:24s} {nbytes[k] / 1e6:7.1f} {med:10.1f} {min(times[k]):8.1f} {max(times[k]):8.1f} "
                     f"{nbytes[k] / med / 1e3:7.1f} {ymed:8.1f} {med / ymed:7.2f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_file:
        Path(out_file).parent.mkdir(parents=True, exist_ok=True)
        Path(out_file).write_text(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
