"""Multi-Krum's three kernels against mf_fedavg_reduce_trimmed (median) on the same gathered image.

The image is N client buckets of the c4 engine's trainable size at J = 9 (n16 + n32 + 2 floats, 55 MB each), each
client the same weights plus an update of its own and one client far off.  The launches of the four kernels alternate
in one process, every launch is timed with device events, and the medians after the warm-up are reported.  Bytes:
mf_krum_pairwise and the median read N * n floats (the median writes n more); mf_fedavg_reduce_selected reads the
m' selected rows and writes n; mf_krum_select reads N^2 doubles.  No pass mark: the numbers are a record.

    python tests/diagnostics/krum_bench.py [--clients 8 32 64] [--rounds 20] [--warmup 5] [--out LOG]
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("krum_bench: needs an MI355X (no timing without a device)")
    dev = torch.device("cuda:0")
    n = N16 + N32 + 2
    lines = []
    for nc in args.clients:
        g = torch.Generator(device=dev).manual_seed(nc)
        img = torch.randn(n, device=dev, generator=g).repeat(nc, 1)
        for c in range(nc):
            img[c].add_(torch.randn(n, device=dev, generator=g), alpha=-5.0 if c == 1 else 1e-2)
        img[:, n - 2:] = 1.0
        ws = torch.zeros(ops.krum_ws_bytes(nc, n) // 8, device=dev, dtype=torch.float64)
        D = torch.zeros(nc * nc, device=dev, dtype=torch.float64)
        sel = torch.zeros(nc, device=dev, dtype=torch.int32)
        scores = torch.zeros(nc, device=dev, dtype=torch.float64)
        counts = torch.zeros(3, device=dev, dtype=torch.int32)
        out_sel, out_med = torch.empty(n, device=dev), torch.empty(n, device=dev)
        calls = {"pairwise": lambda: ops.krum_pairwise(img.view(-1), nc, n, ws, D),
                 "select": lambda: ops.krum_select(D, nc, 1, 0, sel, scores, counts),
                 "reduce_selected": lambda: ops.fedavg_reduce_selected(img.view(-1), nc, sel, n - 1, out_sel),
                 "median": lambda: ops.fedavg_reduce_trimmed(img.view(-1), nc, ops.MEDIAN_TRIM, n - 1, out_med)}
        us = {k: [] for k in calls}
        for r in range(args.warmup + args.rounds):
            for k, fn in calls.items():  # alternated: the kernels see the same machine state
                t = timed(fn)
                if r >= args.warmup:
                    us[k].append(t)
        # the results are what they should be on this image: the far client alone is dropped, and the distances and
        # the mean agree with torch over the first 2^20 coordinates (fp32 / fp64 rounding apart)
        kept = [c for c in range(nc) if int(sel[c])]
        assert kept == [c for c in range(nc) if c != 1] and counts.tolist() == [nc, 1, nc - 1], (kept, counts.tolist())
        assert float(out_sel[n - 1]) == nc and float(out_sel[n - 2]) == 1.0
        part = img[:, :1 << 20]
        want = part[kept].double().mean(0)
        assert torch.allclose(out_sel[:1 << 20].double(), want, rtol=1e-5, atol=1e-6)
        d02 = ((img[0] - img[2]).double() ** 2).sum()
        assert abs(float(D[2]) - float(d02)) <= 1e-9 * float(d02) and float(D[0]) == 0.0
        mprime = len(kept)
        nbytes = {"pairwise": nc * n * 4, "select": nc * nc * 8, "reduce_selected": (mprime + 1) * n * 4,
                  "median": (nc + 1) * n * 4}
        rec = {"clients": nc, "floats_per_client": n, "kept": mprime,
               "ws_MB": round(ws.numel() * 8 / 1e6, 1)}
        for k in calls:
            med = statistics.median(us[k])
            rec[k] = {"median_us": round(med, 1), "min_us": round(min(us[k]), 1), "max_us": round(max(us[k]), 1),
                      "bytes": nbytes[k], "TBps": round(nbytes[k] / med / 1e6, 4)}
        rec["pairwise_over_median"] = round(rec["pairwise"]["median_us"] / rec["median"]["median_us"], 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del img, ws, out_sel, out_med
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
