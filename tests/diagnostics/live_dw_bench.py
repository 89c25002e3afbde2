"""Diagnostic (GPU box): the class-row block's four vision weight gradients and their bias gradients, dead-row form
against the full one (mf_gemm_splitk_live / mf_gemm_splitk, mf_colsum_f16_live / mf_colsum_f16), on operands with one
live row per 199-row sequence (B = 32: K = 6 368); microseconds per call under a hipGraph, ROUNDS separate timings of
each so the spread shows beside the difference.  dW_qkv: only the dQ third of dY (m < 768) has dead rows.
    python live_dw_bench.py [rounds]"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from federated_multi_modal_amd import ops  # noqa: E402


def timeit(fn, reps=20):
    """per-call time of `reps` calls captured in one hipGraph (no host overhead), best of 3 replays"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        s.record()
        g.replay()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) / reps * 1e3)
    return best


def fmt(v):
    return " ".join(f"{x:5.1f}" for x in v) + f"  med {sorted(v)[len(v) // 2]:5.1f} spread {max(v) - min(v):4.1f}"


dev = torch.device("cuda:0")
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
L, B = 199, 32
K = L * B
for name, M, N, m_live in [("v.dW_fc", 3072, 768, 3072), ("v.dW_proj", 768, 3072, 768), ("v.dW_qkv", 2304, 768, 768),
                           ("v.dW_out", 768, 768, 768)]:
    dY = torch.zeros(K, M, device=dev, dtype=torch.float16)
    dY[::L] = torch.randn(B, M, device=dev).half()
    dY[:, m_live:] = torch.randn(K, M - m_live, device=dev).half()
    X = torch.randn(K, N, device=dev).half()
    C, C2 = (torch.empty(M, N, device=dev, dtype=torch.float16) for _ in range(2))
    ws = torch.empty(ops.gemm_splitk_ws_floats(M, N, K), device=dev)
    full = lambda: ops.gemm_splitk(dY, X, C, ws, a_kmajor=True, b_kmajor=True)
    live = lambda: ops.gemm_splitk(dY, X, C2, ws, a_kmajor=True, b_kmajor=True, live=(1, L), m_live=m_live)
    tf, tl = [], []
    for _ in range(rounds):  # alternated
        tf.append(timeit(full))
        tl.append(timeit(live))
    assert torch.equal(C.view(torch.int16), C2.view(torch.int16))
    print(f"{name:10s} full {fmt(tf)}\n{'':10s} live {fmt(tl)}", flush=True)
    if m_live == M:
        db, db2 = (torch.empty(M, device=dev, dtype=torch.float16) for _ in range(2))
        cws = torch.empty(ops.colsum_ws_floats(K, M), device=dev)
        cases = [("colsum full", lambda: ops.colsum(dY, db, cws)),
                 ("colsum live", lambda: ops.colsum(dY, db2, cws, live=(1, L))),
                 ("partials only, full", lambda: ops.colsum(dY, None, cws)),
                 ("partials only, live", lambda: ops.colsum(dY, None, cws, live=(1, L)))]
        t = {n: [] for n, _ in cases}
        for _ in range(rounds):
            for n, f in cases:
                t[n].append(timeit(f))
        assert torch.equal(db.view(torch.int16), db2.view(torch.int16))
        for n, _ in cases:
            print(f"{'':10s} {n:20s} C={M:5d} {fmt(t[n])}", flush=True)
