"""Where the bounds of tests/test_attention_kernels_gpu.py come from, and proof that they bite.  CPU only:

    python tests/diagnostics/attention_bounds.py [figures] [small] [mutations]

`restate` is the attention kernels' arithmetic with their documented rounding points, in torch on the CPU:

  forward    scores S = Q K^T as fp32 sums of exact fp16 products, m = row max of S;
             P = exp2(fma(S, c, -m c)) in fp32 with c = fp32(log2(e) / 8) (the 1 / 8 scale applied in fp32);
             l = row sum of the fp32 P;  P rounded to fp16;  P V accumulated in fp32;  out = fp16(acc / l);
             lse = m / 8 + log(l) in fp32
  backward   D = sum_d fp16(O) fp16(dO) in fp32;  P = exp2(fma(S, c, -fp32(lse log2(e)))) in fp32;
             dP = dO V^T in fp32;  dS = P (dP - D);  P and dS rounded to fp16;  dV = P^T dO, dK = dS^T Q, dQ = dS K
             accumulated in fp32;  dQ and dK scaled by 1 / 8 and rounded to fp16.

What it does not restate: the order of the fp32 sums inside an MFMA and across key chunks, and the hardware's exp2 and
log.  The tests allow 4 x the figures printed here for those.

`figures` prints, per case of the tests' lists (same generators, same seeds) and per output, the restatement's
error against fp64 in the tests' own units (figures() there), then the worst of each bound group next to the constant
the test file holds.  `small` prints the small-gradient table of DESIGN.md (CASE5).  `mutations` applies six
plausible kernel mistakes to the restatement and asserts that each one breaks at least one bound on at least one
listed case.  Five do so on the plain forward + backward cases.  The sixth, D from the backward's own fp32 O instead
of the stored fp16 O, is *closer* to fp64 than the kernels are (its dq / dk figures are 0.1 to 1.4 x theirs: D from
the rounded O is the largest single error term of a peaked softmax), so no upper bound against the fp64 gradient can
see it; it breaks the bounds of CASE8, where the backward is handed -out and D has to follow the buffer.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import test_attention_kernels_gpu as T  # noqa: E402

LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)
C2 = torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32)  # the kernels' kLog2eScale

MUTATIONS = ("causal_off_by_one", "padded_key_unmasked", "last_tile_skipped", "scale_2^-8", "lse_max_unscaled",
             "D_from_fp32_out")


def fma(a, b, c):
    """fp32 fma: the product of two fp32 is exact in fp64, the sum is rounded once more (to 53, then 24 bits)."""
    return (a.double() * b.double() + c.double()).float()


def restate(qkv, dout, N, L, H, causal, mut=None, round_ds=True, negate_out=False):
    """out (fp16), lse (fp32), dq, dk, dv (fp16) as [N, H, L, .], the kernels' rounding points; `mut` one of MUTATIONS.
    round_ds = False keeps P and dS in fp32 for the backward's products (what the fp16 operands cost, `small`);
    negate_out hands the backward -out (CASE8), which a backward that takes D from its own fp32 O does not notice."""
    q, k, v = (t.float() for t in T.heads(qkv, N, L, H))
    do = T.heads(dout, N, L, H)[0].float() if dout is not None else None
    Lk = L
    if mut == "padded_key_unmasked":  # key index L, stage_rows' copy of row L - 1, takes part
        k = torch.cat([k, k[:, :, -1:]], 2)
        v = torch.cat([v, v[:, :, -1:]], 2)
        Lk = L + 1
    dead = torch.zeros(L, Lk, dtype=torch.bool)
    if causal:
        dead = torch.ones(L, Lk, dtype=torch.bool).triu(1)
        if mut == "causal_off_by_one" and L >= 2:
            dead[L - 2, L - 1] = False  # key L - 1 visible one row too early
    if mut == "last_tile_skipped":
        dead = dead.clone()
        dead[:, 16 * ((L + 15) // 16 - 1):] = True
    c2 = C2 * (1 + 2.0 ** -8) if mut == "scale_2^-8" else C2
    ninf = torch.tensor(float("-inf"))

    s = q @ k.transpose(-1, -2)  # raw scores, fp32
    sm = torch.where(dead, ninf, s)
    m = sm.amax(-1, keepdim=True)
    p = torch.where(dead, torch.zeros(()), torch.exp2(fma(s, c2, -m * c2)))
    l = p.sum(-1, keepdim=True)
    acc = p.half().float() @ v
    o32 = acc * (1.0 / l)
    out = o32.half()
    scale = c2 / LOG2E if mut == "scale_2^-8" else torch.tensor(0.125)
    lse = (m if mut == "lse_max_unscaled" else m * scale) + torch.log(l)
    res = dict(out=out, lse=lse.squeeze(-1))
    if do is None:
        return res

    o_given = -out.float() if negate_out else out.float()
    d = ((o32 if mut == "D_from_fp32_out" else o_given) * do).sum(-1, keepdim=True)
    pb = torch.where(dead, torch.zeros(()), torch.exp2(fma(s, c2, -(lse * LOG2E))))
    dp = do @ v.transpose(-1, -2)
    ds = pb * (dp - d)
    p16, ds16 = (pb.half().float(), ds.half().float()) if round_ds else (pb, ds)
    dv = p16.transpose(-1, -2) @ do
    dk = ds16.transpose(-1, -2) @ q
    dq = ds16 @ k
    res.update(dq=(dq * 0.125).half(), dk=(dk[:, :, :L] * 0.125).half(), dv=dv[:, :, :L].half())
    return res


def fused_qkv(N, L, H):
    """The in-projection of a CASE7 shape on the CPU (fp32 accumulate, fp16(acc + bias))."""
    x, w, b = T.host_inputs_fused(N, L, H)
    return (x.float() @ w.float().t() + b.float()).half()


def edge_slices(c):
    """The sequences of a many-head case the tests compare in full: the first and the last two."""
    return [(0, 2), (c.N - 2, 2)]


def listed_cases():
    """(group, name, qkv, dout, N, L, H, causal) of every comparison the tests make against fp64; group "given_out":
    the backward is handed -out (CASE8)."""
    for c in T.CASE1 + T.CASE2 + T.CASE6:
        qkv, dout = T.host_inputs(c)
        yield "unit", f"case{c.tag} {T._id(c)}", qkv, dout, c.N, c.L, c.H, c.causal
    for c in T.CASE3_SPLIT + [T.CASE3_TEXT, T.CASE3_PERSISTENT]:
        qkv, dout = T.host_inputs(c)
        for s0, n in edge_slices(c)[:1 if c is T.CASE3_PERSISTENT else 2]:
            rows = slice(s0 * c.L, (s0 + n) * c.L)
            yield "unit", f"case3 {T._id(c)} seq {s0}..", qkv[rows], dout[rows], n, c.L, c.H, c.causal
    for c in T.CASE4_PEAKED + T.CASE4_FLAT:
        qkv, dout = T.host_inputs(c)
        yield ("peaked" if c.qk_scale > 1 else "flat"), f"case4 {T._id(c)}", qkv, dout, c.N, c.L, c.H, c.causal
    for c in T.CASE5:
        qkv, dout = T.host_inputs(c)
        for e in T.CASE5_EXPONENTS:
            dout_e = (dout.float() * 2.0 ** e).half()
            yield ("unit" if e == 0 else f"small{e}"), f"case5 {T._id(c)} 2^{e}", qkv, dout_e, c.N, c.L, c.H, c.causal
    for c in T.CASE8:
        qkv, dout = T.host_inputs(c)
        yield "given_out", f"case8 {T._id(c)} -out", qkv, dout, c.N, c.L, c.H, c.causal
    for (N, L, H, causal) in T.CASE7:
        yield "unit", f"case7 N{N} L{L} H{H}", fused_qkv(N, L, H), None, N, L, H, causal


def bound_of(group):
    if group.startswith("small"):
        b = dict(T.BOUND_UNIT)
        b.update(T.BOUND_SMALL[int(group[5:])])
        return b
    return dict(unit=T.BOUND_UNIT, peaked=T.BOUND_PEAKED, flat=T.BOUND_FLAT, given_out=T.BOUND_GIVEN_OUT)[group]


def both(group, qkv, dout, N, L, H, causal, mut=None):
    """The restatement (with a mutation) and its fp64 reference in the layout figures() takes."""
    if group != "given_out":
        return restate(qkv, dout, N, L, H, causal, mut), None
    got = restate(qkv, dout, N, L, H, causal, mut, negate_out=True)
    given = -got["out"].permute(0, 2, 1, 3).reshape(N * L, 64 * H)  # [N, H, L, 64] -> [N L, D]
    return {k: got[k] for k in ("dq", "dk", "dv")}, T.ref64_given_out(qkv, dout, given, N, L, H, causal)


def rel_l2(got, ref, k):
    return ((got[k].double() - ref[k]).norm() / ref[k].norm().clamp_min(1e-300)).item()


def figures_part():
    worst = {}
    keys = ("lse", "lse_rel", "out", "dq", "dk", "dv")
    print(f"{'case':46s}" + "".join(f"{k:>11s}" for k in keys) + "   rel L2 dq / dk / dv")
    for group, name, qkv, dout, N, L, H, causal in listed_cases():
        got, ref = both(group, qkv, dout, N, L, H, causal)
        ref = ref or T.ref64(qkv, dout, N, L, H, causal)
        f = T.figures(got, ref)
        w = worst.setdefault(group, {})
        for k in keys:
            if k in f:
                w[k] = max(w.get(k, 0.0), f[k])
        l2 = "  ".join(f"{rel_l2(got, ref, k):.2e}" for k in ("dq", "dk", "dv") if k in got and ref[k].abs().max() > 0)
        print(f"{name:46s}" + "".join(f"{f[k]:11.3e}" if k in f else " " * 11 for k in keys) + "   " + l2)
    print("\nworst per group; the test file's constant is 4 x this figure:")
    for group, w in worst.items():
        b = bound_of(group)
        own = T.BOUND_SMALL[int(group[5:])] if group.startswith("small") else b  # out and lse there: the unit group's
        for k in keys:
            if k in own:
                note = "" if abs(b[k] / (4 * w[k]) - 1) < 0.01 else "   <-- the constant does not quote this figure"
                print(f"  {group:9s} {k:8s} {w[k]:.3e}   4 x = {4 * w[k]:.3e}   constant {b[k]:.3e}{note}")


def mutations_part():
    cases = list(listed_cases())
    refs = {}
    for mut in MUTATIONS:
        broken = []
        for i, (group, name, qkv, dout, N, L, H, causal) in enumerate(cases):
            if mut == "causal_off_by_one" and not (causal and L >= 2):
                continue
            if mut == "padded_key_unmasked" and causal:  # the causal mask hides key L from every row
                continue
            if mut == "last_tile_skipped" and L <= 16:   # nothing would be left
                continue
            if mut == "D_from_fp32_out" and dout is None:
                continue
            got, ref = both(group, qkv, dout, N, L, H, causal, mut)
            if ref is None:
                if i not in refs:
                    refs[i] = T.ref64(qkv, dout, N, L, H, causal)
                ref = refs[i]
            f = T.figures(got, ref)
            b = bound_of(group)
            over = [f"{k} {f[k]:.2e} > {b[k]:.2e}" for k in b if k in f and not f[k] <= b[k]]
            if over:
                broken.append((name, over))
        print(f"{mut}: breaks a bound on {len(broken)} cases" + (f", e.g. {broken[0][0]}: {'; '.join(broken[0][1])}"
                                                                  if broken else ""))
        assert broken, f"mutation {mut} passes every bound: the bounds do not bite"


def small_part():
    """CASE5: relative L2 error of dq / dk / dv against fp64 per dout scale, with P and dS rounded to fp16 as the
    kernels do and with both kept in fp32 (the outputs are rounded to fp16 either way)."""
    print(f"{'case':40s}  fp16 P, dS: dq       dk       dv        fp32 P, dS: dq       dk       dv      mean |dO|")
    for group, name, qkv, dout, N, L, H, causal in listed_cases():
        if not name.startswith("case5"):
            continue
        ref = T.ref64(qkv, dout, N, L, H, causal)
        a = restate(qkv, dout, N, L, H, causal)
        b = restate(qkv, dout, N, L, H, causal, round_ds=False)
        row = ["  ".join(f"{rel_l2(r, ref, k):.2e}" for k in ("dq", "dk", "dv")) for r in (a, b)]
        print(f"{name:40s}  {row[0]}              {row[1]}    {dout.float().abs().mean():.2e}")


if __name__ == "__main__":
    torch.manual_seed(0)
    parts = sys.argv[1:] or ["figures", "small", "mutations"]
    if "figures" in parts:
        figures_part()
    if "small" in parts:
        small_part()
    if "mutations" in parts:
        mutations_part()
