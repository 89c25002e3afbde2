"""Diagnostic (GPU box): the top-k uplink kernels at the c4 trainable size (J = 9: 13 856 770 coordinates, half of them
taken as fp16 and half as fp32 trainables, one destination rank), timed with HIP events and alternated in the same
process with the int8 pair, which reads the same inputs and is the yardstick: mf_topk_select (k = 8, error feedback)
against mf_compress_quantize (nearest, error feedback), mf_topk_decode against mf_compress_decode (plain layout), and
the selection at k = 1 and 64 beside them (its search takes 39 steps whatever k).  10 warm-up rounds, medians of 40.
Not a gate: the kernels run once per client and round, beside seconds of training.

    python topk_bench.py [out_file]
"""
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from federated_multi_modal_amd import ops  # noqa: E402

N = 13_856_770
WARMUP, REPS = 10, 40
KS = (8, 1, 64)


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
    chunk8 = ops.compress_chunk_bytes(S)
    chunks = {k: ops.topk_chunk_bytes(S, k) for k in KS}
    image8 = torch.zeros(1, 1, chunk8, dtype=torch.uint8, device=dev)
    images = {k: torch.zeros(1, 1, chunks[k], dtype=torch.uint8, device=dev) for k in KS}
    e_in, e_out = 1e-4 * torch.randn(N, generator=g).to(dev), torch.zeros(N, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros(S, device=dev)
    weights = 2 * (2 * n16 + 4 * n32)  # the weights and the global copy, read

    def select(k):
        ops.topk_select(p16, p32, g16, g32, e_in, e_out, flag, None, k, images[k], 0, S)

    runs = {"int8 quantize nearest": (lambda: ops.compress_quantize(p16, p32, g16, g32, e_in, e_out, flag, None, "nearest",
                                                                   1234, 1, 0, image8, 0, S), weights + 8 * N + chunk8)}
    for k in KS:
        runs[f"topk select k={k}"] = (lambda k=k: select(k), weights + 8 * N + chunks[k])
    runs["int8 decode"] = (lambda: ops.compress_decode(image8.view(-1), 1, chunk8, S, 0, 0, g16, g32, "plain", out, S),
                           chunk8 + weights // 2 + 4 * S)
    for k in KS:
        runs[f"topk decode k={k}"] = (lambda k=k: ops.topk_decode(images[k].view(-1), 1, chunks[k], S, 0, 0, g16, g32,
                                                                  "plain", out, S, k), chunks[k] + weights // 2 + 4 * S)
    times = {name: [] for name in runs}
    for it in range(WARMUP + REPS):
        for name, (fn, _) in runs.items():  # alternated: every kernel sees the same clocks and the same neighbours
            t = timed(fn)
            if it >= WARMUP:
                times[name].append(t)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    lines = [f"{torch.cuda.get_device_name(0)}; {N} coordinates, S = {S}, int8 chunk = {chunk8} bytes, top-k chunks = "
             f"{chunks}; {WARMUP} warm-up rounds, medians of {REPS}, alternated",
             f"{'kernel':24s} {'MB':>7s} {'median us':>10s} {'min us':>8s} {'max us':>8s} {'GB/s':>7s} {'x int8':>7s}"]
    for name, (_, nbytes) in runs.items():
        base = med["int8 quantize nearest" if "select" in name or "quantize" in name else "int8 decode"]
        lines.append(f"{name:24s} {nbytes / 1e6:7.1f} {med[name]:10.1f} {min(times[name]):8.1f} {max(times[name]):8.1f} "
                     f"{nbytes / med[name] / 1e3:7.1f} {med[name] / base:7.2f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_file:
        Path(out_file).parent.mkdir(parents=True, exist_ok=True)
        Path(out_file).write_text(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
