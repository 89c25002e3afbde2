"""The host restatement of Multi-Krum (Blanchard et al., NeurIPS 2017; El Mhamdi et al., ICML 2018), written from the
contract in include/mapfed.h, not from the kernels: the literal loops, in numpy / torch on the CPU.

  host_pairwise       D[i][j] = sum_t (double)(x_i[t] - x_j[t])^2: fp32 subtract, fp64 square and sum
  host_select         combine the parts in order, presence from the diagonal, f', q, the scores, m', the selection
  host_selected_mean  sequential fp32 adds over the selected clients in client order, one division
  stable_selection    the precondition of every bit-for-bit comparison across layouts: the selection survives
                      perturbations of D a thousand times larger than any two summation orders can differ by
  gamma2              2 * gamma_n, the relative bound on two summation orders of n non-negative fp64 terms"""
import numpy as np
import torch


def gamma2(n):
    u = n * 2.0 ** -53
    return 2.0 * u / (1.0 - u)


def host_pairwise(x):
    """x: [clients, n] fp32 (torch or numpy).  Returns the [clients, clients] fp64 matrix; the summation order is
    numpy's, so it agrees with any other order to gamma2(n) relative."""
    x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    nc = x.shape[0]
    D = np.zeros((nc, nc), np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(nc):
            d = (x[i][None, :] - x[i:]).astype(np.float64)  # one fp32 subtract, then exact in fp64
            D[i, i:] = (d * d).sum(axis=1)
            D[i:, i] = D[i, i:]
    return D


def host_select(parts, f, m):
    """parts: [nparts, clients, clients] fp64 (or one matrix).  Returns (selected: list of 0 / 1, scores: fp64 array
    with NaN for an absent client, (p, f', m'), the combined D)."""
    parts = np.asarray(parts, np.float64)
    if parts.ndim == 2:
        parts = parts[None]
    with np.errstate(invalid="ignore"):
        D = parts[0].copy()
        for part in parts[1:]:  # rank order, sequential fp64 adds
            D = D + part
    nc = D.shape[0]
    present = [i for i in range(nc) if not np.isnan(D[i, i])]
    p = len(present)
    fe = max(min(f, (p - 3) // 2), 0)
    q = max(p - fe - 2, 0)
    me = p - fe if m == 0 else min(m, p - fe)
    scores = np.full(nc, np.nan, np.float64)
    for i in present:
        terms = sorted((D[i, j], j) for j in present if j != i)[:q]
        s = np.float64(0.0)
        for t, (v, _) in enumerate(terms):
            s = v if t == 0 else s + v
        scores[i] = s
    keep = sorted((scores[i], i) for i in present)[:me]
    selected = [0] * nc
    for _, i in keep:
        selected[i] = 1
    return selected, scores, (p, fe, me), D


def host_selected_mean(g, selected, count_pos=-1):
    """g: [clients, n] fp32 torch on the CPU.  The selected rows summed in client order from the first selected one,
    one fp32 add each, divided by their number; nobody selected: +0; out[count_pos] = the non-NaN values there."""
    g = g.detach().contiguous()
    rows = [c for c, s in enumerate(selected) if s]
    if rows:
        acc = g[rows[0]].clone()
        for c in rows[1:]:
            acc = acc + g[c]
        out = acc / torch.tensor(float(len(rows)), dtype=torch.float32)
    else:
        out = torch.zeros(g.shape[1], dtype=torch.float32)
    if count_pos >= 0:
        out[count_pos] = float((~torch.isnan(g[:, count_pos])).sum())
    return out


def stable_selection(D, f, m):
    """Asserts that 8 seeded symmetric perturbations D * (1 + 1e-9 U), U in [-1, 1], select what D selects, and
    returns that selection.  1e-9 is more than a thousand times gamma2(n) for n below 2^22, so a selection that
    passes cannot depend on the order the distances were summed in."""
    D = np.asarray(D, np.float64)
    want = host_select(D, f, m)[0]
    for seed in range(8):
        u = np.random.default_rng(7000 + seed).uniform(-1.0, 1.0, D.shape)
        u = np.triu(u) + np.triu(u, 1).T
        with np.errstate(invalid="ignore"):
            got = host_select(D * (1.0 + 1e-9 * u), f, m)[0]
        assert got == want, (seed, got, want)
    return want
