"""Where the bounds of tests/test_reduction_kernels_gpu.py come from.  CPU only:

    python tests/diagnostics/reduction_bounds.py [ln] [head | head-search] [clip]

Each part restates a kernel's arithmetic in fp32 (numpy, one rounding per operation, the kernel's summation
grouping) on the very inputs the test uses and measures it against fp64.  The test allows 4x what is printed here
(another legal fp32 summation order); the head's stages have a fixed bound (one fp16 ulp, 1 % beyond half an ulp)
and are only shown to stay under it.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import test_reduction_kernels_gpu as R  # noqa: E402
from test_kernels_gpu import ulp16  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------ LayerNorm
def half_sum(v):
    """half_sum of layernorm.hip on [rows, 32]: butterflies xor 16..1, every lane ends with the same bits."""
    idx = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        v = v + v[:, idx ^ o]
    return v[:, 0]


def two_partials(terms):
    """terms [rows, CH, 32, 8] -> the e < 4 and e >= 4 partial of each lane, summed j outer, e inner, then
    half_sum(s0) + half_sum(s1)."""
    rows, CH = terms.shape[:2]
    s0, s1 = np.zeros((rows, 32), f32), np.zeros((rows, 32), f32)
    for j in range(CH):
        for e in range(8):
            if e < 4:
                s0 = s0 + terms[:, j, :, e]
            else:
                s1 = s1 + terms[:, j, :, e]
    return half_sum(s0) + half_sum(s1)


def ln_fwd2(x16):
    """mean, rstd of ln_fwd2_kernel."""
    rows, D = x16.shape
    v = x16.astype(f32).reshape(rows, D // 256, 32, 8)
    mean = two_partials(v) / f32(D)
    d = v - mean[:, None, None, None]
    var = two_partials(d * d) / f32(D)
    rstd = f32(1.0) / np.sqrt(np.maximum(var, f32(0)) + f32(1e-5))
    return mean, rstd


def ln_bwd2_dx(x16, dy16, gamma, mean, rstd):
    """dx (fp16) of ln_bwd2_kernel without a residual gradient."""
    rows, D = x16.shape
    shp = (rows, D // 256, 32, 8)
    xv, dv = x16.astype(f32).reshape(shp), dy16.astype(f32).reshape(shp)
    gv = gamma.astype(f32).reshape(1, *shp[1:])
    dg = dv * gv
    sdg, sdgx = two_partials(dg), two_partials(dg * xv)
    invD = f32(1.0) / f32(D)
    b = (sdg * mean - sdgx) * rstd * rstd * rstd * invD
    c = -b * mean - sdg * rstd * invD
    m = lambda a: a[:, None, None, None]  # noqa: E731
    t = ((m(rstd) * dv) * gv + m(b) * xv) + m(c)
    return t.astype(np.float16).reshape(rows, D)


def ln_part():
    wm = wr = 0.0
    cases = [(f"D={D} rows={rows}", R._ln_case_host(D, rows)[:4]) for D in R.LN_D for rows in R.LN_ROWS]
    cases += [(f"edge rows D={D}", R._ln_edge_rows(D)) for D in R.LN_D]
    for name, (x, gamma, beta, dy) in cases:
        ref = R._ln_ref64(x, gamma, beta, dy)
        mean, rstd = ln_fwd2(x.numpy())
        em = ((torch.from_numpy(mean).double() - ref["mean"]).abs() / ref["absmean"].clamp_min(1e-30)).max().item()
        er = ((torch.from_numpy(rstd).double() - ref["rstd"]).abs() / ref["rstd"]).max().item()
        print(f"ln {name}: mean err / mean|x| {em:.3e}, rstd rel err {er:.3e}")
        wm, wr = max(wm, em), max(wr, er)
        if name.startswith("edge"):
            dx = ln_bwd2_dx(x.numpy(), dy.numpy(), gamma.numpy(), mean, rstd)
            unit = ulp16(ref["dx"].abs().max(1).values)
            ulps = (torch.from_numpy(dx).double() - ref["dx"]).abs().max(1).values / unit
            print(f"   dx err in fp16 ulps of the row maximum: offset row {ulps[R.EDGE_OFFSET]:.3f}, outlier row "
                  f"{ulps[R.EDGE_OUTLIER]:.3f}, all rows {[round(v, 3) for v in ulps.tolist()]}")
            # the same with b formed from dg (x - mean): what the cancellation in b costs
            xd, m64 = x.double(), ref["mean"][:, None]
            dgd = dy.double() * gamma.double()
            b_exact = -(dgd * (xd - m64)).sum(1) * ref["rstd"] ** 3 / x.shape[1]
            sdg = torch.from_numpy(two_partials((dy.numpy().astype(f32) * gamma.numpy()).reshape(16, -1, 32, 8)))
            b32 = (sdg * torch.from_numpy(mean) - torch.from_numpy(two_partials(
                ((dy.numpy().astype(f32) * gamma.numpy()) * x.numpy().astype(f32)).reshape(16, -1, 32, 8)))) \
                * torch.from_numpy(rstd) ** 3 / x.shape[1]
            rel = ((b32.double() - b_exact).abs() / b_exact.abs().clamp_min(1e-300))
            print(f"   rel err of b: offset row {rel[R.EDGE_OFFSET]:.2e}, outlier row {rel[R.EDGE_OUTLIER]:.2e}")
    print(f"ln worst: mean {wm:.3e}, rstd {wr:.3e}")


# ------------------------------------------------------------------------------------------- CLIP head and loss
class Record:
    def __init__(self):
        self.rows = []

    def __call__(self, out, ref, max_ulp=1.0, frac=1e-2, what="", floor=2e-5):
        unit = torch.maximum(ulp16(ref), torch.tensor(floor * ref.abs().max().item()))
        d = (out.float() - ref.float()).abs() / unit
        self.rows.append((what, d.max().item(), (d > 0.51).float().mean().item(), d.numel()))
        R.assert_ulps(out, ref, max_ulp, frac, what, floor)


def head_cpu(B, K, D, soft, seed, label=None, perm=None, zero_row=None):
    """The head in fp32 on the CPU, stage by stage (the test's references at T = float32).  perm: a permutation of
    the feature axis, i.e. another fp32 summation order of the same mathematical case."""
    T = torch.float32
    img, txt, lab, q, ls = R.head_inputs(B, K, D, seed)
    if label is not None:
        lab = torch.tensor(label)
    if zero_row is not None:
        img[zero_row] = 0.0
    if perm is not None:
        img, txt = img[:, perm].contiguous(), txt[:, perm].contiguous()
    h = dict(img=img, txt=txt, label=lab, q=q, ls=ls)
    sc = R._scale(ls)
    h["norms"] = R.ref_norms(torch.cat([img, txt]), T)
    h["img_n"] = R.ref_normalized(img, h["norms"][:B], T)
    h["txt_n"] = R.ref_normalized(txt, h["norms"][B:], T)
    h["mm"] = R.ref_mm(h["img_n"], h["txt_n"], T)
    h["logits"] = (sc * h["mm"].float()).half()
    if soft:
        tgt = R.ref_soft_target(q, h["txt_n"], T)
        r = R.ref_loss_soft(h["logits"], h["img_n"], tgt, q, sc, T)
        h["soft_ws"] = torch.cat([tgt.reshape(-1), r["gtgt"].reshape(-1)])
        h.update(dmm=r["dmm"], cos_ws=r["cos_ws"], loss=torch.cat([r["loss"], torch.zeros(1)]))
        h["dimg_n"] = R.ref_dimg_n(h["dmm"], h["img_n"], h["txt_n"], tgt, h["cos_ws"], T)
        h["dtxt_n"] = R.ref_dtxt_soft(h["dmm"], h["img_n"], q, r["gtgt"], T)
    else:
        r = R.ref_loss_hard(h["logits"], h["img_n"], h["txt_n"], lab, sc, T)
        h.update(dmm=r["dmm"], cos_ws=r["cos_ws"], loss=torch.cat([r["loss"], torch.zeros(1)]))
        h["dimg_n"] = R.ref_dimg_n(h["dmm"], h["img_n"], h["txt_n"], h["txt_n"][lab], h["cos_ws"], T)
        h["dtxt_n"] = R.ref_dtxt_n(h["dmm"], h["img_n"], h["txt_n"], lab, h["cos_ws"], T)
    h["dimg"] = R.ref_normalize_bwd(img, h["dimg_n"], h["norms"][:B], T)
    h["dtxt"] = R.ref_normalize_bwd(txt, h["dtxt_n"], h["norms"][B:], T)
    return h


def head_runs():
    runs = [(s, False, None, None) for s in R.HEAD_SHAPES] + [(s, True, None, None) for s in R.HEAD_SOFT_SHAPES]
    runs += [(R.HEAD_SOFT_B64, True, None, None)]
    runs += [(R.HEAD_SHARED, False, lab, None) for lab in R.HEAD_SHARED_LABELS]
    runs += [(R.HEAD_ZERO_ROW, False, None, 1)]
    return runs


def head_check(shape, soft, seed, lab, zero_row, perm):
    h = head_cpu(*shape, soft, seed, lab, perm, zero_row)
    rec = Record()
    R.check_forward_stages(h, torch.float64, rec)
    if zero_row is not None:  # the test looks at the forward and the loss only
        r = R.ref_loss_hard(h["logits"], h["img_n"], h["txt_n"], h["label"], R._scale(h["ls"]), torch.float64)
        rec(h["loss"][:3], r["loss"], 1.0, what="loss with a zero row")
        return rec.rows
    (R.check_soft_stages if soft else R.check_hard_stages)(h, torch.float64, rec)
    R._check_end_to_end(h, soft)
    return rec.rows


def head_perms(D):
    g = torch.Generator().manual_seed(D)
    return [None, torch.arange(D - 1, -1, -1), torch.randperm(D, generator=g), torch.randperm(D, generator=g)]


def head_part(search=False):
    """Every stage-checked case of the test at its seed (R.head_seed), in four fp32 summation orders (the feature
    axis as drawn, reversed and twice shuffled).  A seed is kept only if all four stay under the bound: a case with
    an element that sits on an fp16 rounding boundary to within the fp32 summation error fails about half of them.
    `search` lists the first such seed of every case."""
    worst, wfrac = 0.0, 0.0
    for shape, soft, lab, zero_row in head_runs():
        key = (shape, soft, tuple(lab) if lab else None)
        seeds = range(1, 60) if search else [R.head_seed(*key)]
        for seed in seeds:
            try:
                rows = [r for perm in head_perms(shape[2]) for r in head_check(shape, soft, seed, lab, zero_row, perm)]
            except AssertionError as e:
                print(f"head {key} seed {seed}: {e}")
                continue
            w, fr = max(r[1] for r in rows), max(r[2] for r in rows)
            print(f"head {key} seed {seed}: worst {w:.2f} ulp, worst fraction beyond half an ulp {fr:.4f}")
            worst, wfrac = max(worst, w), max(wfrac, fr)
            break
    print(f"head worst: {worst:.2f} ulp, fraction {wfrac:.4f}")


# ------------------------------------------------------------------------------------------ gradient-norm clip
def wave_sum64(v):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ o]
    return v[0]


def sumsq_chunk(g, s, e, W):
    """sumsq_chunks_kernel on elements [s, e) of the fp32 copy g of a flat buffer; W = 8 (fp16) or 4 (fp32)."""
    a = min(e, (s + W - 1) // W * W)
    b = max(a, e // W * W)
    acc = np.zeros(256, f32)
    for lo, hi in ((s, a), (b, e)):            # scalar head and tail: thread i - lo
        v = g[lo:hi]
        acc[:hi - lo] = acc[:hi - lo] + v * v
    nv = (b - a) // W
    if nv:
        rounds = -(-nv // 256)
        v = np.zeros((rounds * 256, W), f32)
        v[:nv] = g[a:b].reshape(nv, W)
        v = v.reshape(rounds, 256, W)
        sq = v * v
        for r in range(rounds):
            if W == 8:
                for k in range(8):
                    acc = acc + sq[r, :, k]
            else:
                acc = acc + (((sq[r, :, 0] + sq[r, :, 1]) + sq[r, :, 2]) + sq[r, :, 3])
    red = [wave_sum64(acc[64 * w:64 * w + 64]) for w in range(4)]
    return ((red[0] + red[1]) + red[2]) + red[3]


def clip_coef(part, arr, max_norm=1.0):
    """clip_coef_kernel: tiles of 1024, segmented Hillis-Steele scan, carry."""
    n = len(arr)
    segs, is16 = arr["seg"], arr["is16"]
    carry_val, carry_seg = f32(0), -1
    acc = np.zeros(1024, f32)
    t = np.arange(1024)
    for base in range(0, n, 1024):
        m = min(1024, n - base)
        seg = np.full(1024, -1, np.int64)
        seg[:m] = segs[base:base + m]
        v = np.zeros(1024, f32)
        v[:m] = part[base:base + m]
        off = 1
        while off < 1024:
            prev = np.roll(v, off)
            same = (t >= off) & (np.roll(seg, off) == seg)
            v = v + np.where(same, prev, f32(0))
            off <<= 1
        for i in range(m):
            c = base + i
            if c == n - 1 or segs[c + 1] != seg[i]:
                ss = v[i]
                if seg[i] == carry_seg and seg[0] == seg[i]:
                    ss = ss + carry_val
                nrm = np.sqrt(ss)
                if is16[c]:
                    nrm = f32(np.float16(nrm))
                acc[i] = acc[i] + nrm * nrm
        prev = carry_val if (seg[1023] == carry_seg and seg[0] == seg[1023]) else f32(0)
        carry_val, carry_seg = v[1023] + prev, seg[1023]
    red = [wave_sum64(acc[64 * w:64 * w + 64]) for w in range(16)]
    tot = f32(0)
    for r in red:
        tot = tot + r
    total = np.sqrt(tot)
    coef = f32(max_norm) / (total + f32(1e-6))
    return total, min(coef, f32(1))


def clip_part():
    ce = 8192
    worst32 = 0.0
    for all32 in (False, True):
        segs, arr, n16, n32 = R.clip_table(ce, all32)
        print(f"clip all32={all32}: {len(segs)} segments, {len(arr)} chunks, n16 {n16}, n32 {n32}")
        for scale in (1e-3, 1e-4):
            g16, g32 = R.clip_grads(n16, n32, scale)
            a16, a32 = g16.float().numpy(), g32.numpy()
            part = np.array([sumsq_chunk(a16 if h else a32, s, e, 8 if h else 4) for _, h, s, e in arr.tolist()], f32)
            for cut in (None, 1024, 1025):
                sub = arr if cut is None else arr[:cut]
                total, coef = clip_coef(part[:len(sub)], sub)
                ref, rcoef, share = R.clip_ref64(sub, g16, g32)
                rel = abs(float(total) - ref) / ref
                print(f"   scale {scale} cut {cut}: total {float(total):.9g} vs {ref:.9g} rel err {rel:.3e} "
                      f"(fp16 share bound {share / ref:.3e}), coef {float(coef):.9g} vs {rcoef:.9g}")
                if all32:
                    worst32 = max(worst32, rel)
                else:
                    assert rel <= R.CLIP_F32_BOUND + share / ref
    print(f"clip worst all-fp32 rel err: {worst32:.3e}")


if __name__ == "__main__":
    todo = sys.argv[1:] or ["ln", "head", "clip"]
    if "ln" in todo:
        ln_part()
    if "head" in todo or "head-search" in todo:
        head_part("head-search" in todo)
    if "clip" in todo:
        clip_part()
