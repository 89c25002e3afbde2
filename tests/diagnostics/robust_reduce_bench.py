"""mf_fedavg_reduce_trimmed (median) against mf_fedavg_reduce_ordered on the same gathered image.

The image is N client buckets of the c4 engine's trainable size at J = 9 (n16 + n32 floats, 55 MB each), the launches
of the two kernels alternate in one process, every launch is timed with device events, and the medians after the
warm-up are reported.  Both kernels read N * n floats and write n, so bytes = (N + 1) * n * 4; the robust kernel's
VALU work is counted from its compiled code (instructions per thread / coordinates per thread).

    python tests/diagnostics/robust_reduce_bench.py [--clients 2 8 32] [--rounds 40] [--warmup 10] [--out LOG]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from federated_multi_modal_amd import ops  # noqa: E402

N16, N32 = 10_630_144, 3_226_624  # the c4 engine's trainables at J = 9
HBM_PEAK = 8.0e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[2, 8, 32])
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("robust_reduce_bench: needs an MI355X (no timing without a device)")
    dev = torch.device("cuda:0")
    n = N16 + N32 + 2
    lines = []
    for nc in args.clients:
        g = torch.Generator(device=dev).manual_seed(nc)
        img = torch.randn(nc, n, device=dev, generator=g)
        img[:, n - 2:] = 1.0
        out_sum, out_med = torch.empty(n, device=dev), torch.empty(n, device=dev)
        calls = {"ordered": lambda: ops.fedavg_reduce_ordered(img.view(-1), nc, out_sum),
                 "median": lambda: ops.fedavg_reduce_trimmed(img.view(-1), nc, ops.MEDIAN_TRIM, n - 1, out_med)}
        us = {k: [] for k in calls}
        for r in range(args.warmup + args.rounds):
            for k, fn in calls.items():  # alternated: the two kernels see the same machine state
                t = timed(fn)
                if r >= args.warmup:
                    us[k].append(t)
        # the same image through torch, at the sizes timed: the first 2^20 coordinates
        part = img[:, :1 << 20]
        lo = part.kthvalue((nc + 1) // 2, 0).values
        hi = part.kthvalue(nc // 2 + 1, 0).values
        assert torch.equal(out_med[:1 << 20], (lo + hi) / 2), "median differs from torch.kthvalue's"
        assert torch.equal(out_sum[:1 << 20], part.cumsum(0)[-1]) or nc > 2  # the yardstick ran on this image too
        assert float(out_med[n - 1]) == nc and float(out_med[n - 2]) == 1.0
        nbytes = (nc + 1) * n * 4
        rec = {"clients": nc, "floats_per_client": n, "bytes": nbytes}
        for k in calls:
            med = statistics.median(us[k])
            rec[k] = {"median_us": round(med, 1), "min_us": round(min(us[k]), 1), "max_us": round(max(us[k]), 1),
                      "TBps": round(nbytes / med / 1e6, 3), "of_hbm_peak": round(nbytes / med / 1e6 / (HBM_PEAK / 1e12), 3)}
        rec["median_over_ordered"] = round(rec["median"]["median_us"] / rec["ordered"]["median_us"], 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del img, out_sum, out_med
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
