"""The byte-moving and small kernels of csrc/elementwise.hip and mf_argmax_correct (csrc/head.hip) at their edges,
bit for bit.  Every comparison is torch.equal on whole allocations: each output is a view inside a larger buffer
pre-filled with SENTINEL (guard rows before and after, pad columns where the entry takes a leading dimension), and the
expected buffer is the same allocation with only the view filled in, so a write outside the intended region fails the
same comparison as a wrong value.  (Reads outside a buffer cannot be seen this way.)

Two kinds of reference, named in each test's docstring:
  exact        the operation is a copy, a cast, one fp16 add or an argmax: torch's CPU result;
  restatement  tests/_elementwise_ref.py restates the kernel's fp32 summation grouping in numpy (one rounding per
               operation; the library is built with -ffp-contract=off, every reduction has a fixed order), compared
               bit for bit; the same outputs are then held to fp64 within SUM_UNITS (below).

Which input reaches which branch (read off the kernels and the dispatch conditions of the entry points):

mf_im2col_patch      (B, R, P) = (3, 32, 16), (2, 24, 8), (1, 224, 16): 1 152 / 432 / 18 816 threads, the last block
                     ragged every time (t >= total); fp32 images take the two 16-byte loads + cast, fp16 images the
                     16-byte copy; P = 8 gives G = 3 (py, px not powers of two) and 24 chunks per row
mf_vision_assemble   n_ctx = 0: no shared_ctx rows (null pointer); D = 4: one thread per row, 15..27 threads;
                     D = 260: 975 / 1365 / 1755 threads (not a multiple of 256, 4..7 blocks); l == 0 / l <= G2 / else
mf_text_assemble     L = n_ctx + 1: empty suffix (null pointer); n_ctx = 0: no ctx rows; K = 1 and 5; D = 260, L = 8:
                     520 / 2600 threads (3 / 11 blocks)
mf_prompt_inject_fwd row0 = 0, 1, L - nrows; nrows = 1, 2, L (whole sequence); N * nrows * D = 4 .. 3900 threads
mf_prompt_inject_bwd N = 1: only group 0 has a row; 15: group 15 empty; 16: one row each; 17: group 0 sums two;
                     33: groups 0 sums three, the others two (the n += 16 stride matters from N = 17 on);
                     D = 4: one lane; 252, 260: ragged 256-column block (d < D cuts lanes 63 / 1..63 of the last block);
                     256: full block; 768: three blocks; fp32 / fp16 out, accumulate, zero_rows each both ways
mf_seq_grow / _bwd   ncap = 0 (no caption rows), n_ctx = 0 (no prompt rows, nothing dropped), n_ctx = Lp (nothing
                     kept: keep = 0); D = 8 one thread per row, D = 72 nine; 9 .. 351 threads
mf_seq_scatter       L_live == L_full (a plain strided copy), N = 1, both operands strided
mf_caption_pool      T = 1 (softmax of one), 3, 64 (every lane one score), 65 (lane 0 a second), 77, 128 (the limit);
                     T < 4 leaves waves idle in the score loop; D = 64: one element per lane; 100: ragged lanes 36..63;
                     260: five passes, the last ragged, and a second pass of the 256-thread pooled loop; 512
mf_transpose_f16     (1, 1), (63, 65), (65, 63), (130, 200): ragged tiles (full false by r0 + 64 <= R / c0 + 64 <= C);
                     (64, 64), (128, 192) contiguous and with ld_in = C + 8, ld_out = R + 8: full true (16-byte path);
                     ld_in = C + 2, ld_out = R + 2, in or out one element into its allocation: full false on full
                     tiles, one conjunct each (ld_in % 8, ld_out % 8, in % 16, out % 16)
mf_colsum_f16        R = 1, 15: wave 0 only, short; 16: wave 0 full; 17: wave 1 one row; 63, 64, 65: the 64-row chunk
                     ragged / full / a second chunk of one row; 130: three chunks; C = 4: one lane; 252, 260: ragged
                     256-column block; 256 full; ld = C, C + 4 (rows 8-byte aligned only), C + 8; base 4 elements into
                     the allocation; out fp16 / fp32 (col_reduce_kernel<true / false>, tail loop only: nblk <= 3) / None
mf_small_linear_fwd  I = 1: one lane; 63, 64, 65: lane 63 empty / every lane one / lane 0 two; 512; bias given / null
mf_small_linear_bwd  dX: O = 1: group 0's tail only; 15, 16: tails only (o + 16 < O never holds); 17: group 0 one
                     two-accumulator step; 31, 32: groups 0..14 / 0..15 one step, no tail; 33: group 0 a step and a
                     tail; 48: every group a step and a tail (O % 32 == 16: the case `o + 16 <= O` would regroup);
                     768: 24 steps; I = 63, 65: ragged 64-column block (i < I); accumulate_dx; dX / dW / db null
SmallLinearBatch     entries of M = 1, 2, 16, I = 63, 512, O = 17, 768, fp16 and fp32: blockIdx.y >= d.M,
                     blockIdx.x * 64 >= d.I, t >= d.O * d.I and idx >= d.M * d.O all return early for the small entries;
                     null dX, null dW / db, null bias
mf_argmax_correct    B = 1, 15, 16, 17, 100: 1 / 15 / 16 waves busy, rows wrapping once / six times; K = 1, 63: lanes
                     without a candidate (bi < 0 both ways in the butterfly); 64, 65, 1000; the tie and NaN rows of
                     argmax_rows decide in the lane loop (k, k + 64) or in the cross-lane steps (k = 5 / 70, 70 / 10)
mf_cast_f16_f32      all 65 536 bit patterns (256 blocks); n = 1, 255, 257 (t < n in the first / second block)

Bounds against fp64 come from tests/diagnostics/elementwise_bounds.py, which runs the restatements on these very
inputs on the CPU; see SUM_UNITS and CAPTION_ULPS.
"""
import itertools

import numpy as np
import pytest
import torch

import _elementwise_ref as E
from federated_multi_modal_amd import ops
from federated_multi_modal_amd._lib import MapfedError, call

pytestmark = pytest.mark.gpu

SENTINEL = -7.25  # exact in fp16; the int64 buffers use -7
F16, F32 = torch.float16, torch.float32

# |fp32 sum - fp64 sum| <= SUM_UNITS[family] fp32 ulps of sum |terms| (E.check64), for every restated sum of this
# module.  elementwise_bounds.py, restatement against fp64, worst per family over the cases below: inject-bwd 2.125 (N = 17),
# colsum 1.609 (R = 15, C = 252), the small linears 4.904 (dW in fp32 at M = 16, O = 768: 16 rounded products and 16
# additions; Y 1.863, dX 3.990, db 2.179).  4x margin for another legal fp32 order.
# MI355X: the restatement's figures (every output is bit for bit the restatement's).
SUM_UNITS = dict(inject=4 * 2.125, colsum=4 * 1.609, linear=4 * 4.904)

# |pooled - pooled64| <= CAPTION_ULPS fp16 ulps of the fp64 value, pooled64 being fp64 through the same fp16 rounding
# points before the result's own rounding; see test_caption_pool for the figures elementwise_bounds.py prints.
CAPTION_ULPS = 4 * 0.5


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    """Bitwise equality of two tensors of one dtype, NaN payloads and signed zeros included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def rand32(g, *shape, hi=8):
    """randn scaled by 2^randint(-8, hi) per element, so sums actually round (test_fedavg_reduce_ordered_kernel)."""
    return torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-8, hi, shape, generator=g).float())


def rand16(g, *shape, hi=8):
    return rand32(g, *shape, hi=hi).half()


def gen(*key):
    """A CPU generator seeded from the case's parameters (the same on every host and Python)."""
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


class Guarded:
    """A [rows, cols] view with leading dimension cols + pad, inside an allocation filled with the sentinel: `lead`
    elements, then GUARD rows before and after it (8 rows, so the view's alignment is that of `lead` alone whatever
    the leading dimension).  init: the view's content before the call (default: the sentinel).
    check(expected): the whole allocation equals, bit for bit, the initial allocation with the view set to expected
    (expected None: nothing was written at all)."""

    GUARD = 8

    def __init__(self, dev, rows, cols, dtype=F16, pad=0, lead=0, init=None):
        sent = -7 if dtype == torch.int64 else SENTINEL
        ld = cols + pad
        self.buf = torch.full((lead + (rows + 2 * self.GUARD) * ld,), sent, dtype=dtype, device=dev)
        self.view = self._inner(self.buf, lead, rows, cols, ld)
        assert self.view.data_ptr() % 16 == (lead * self.buf.element_size()) % 16
        if init is not None:
            self.view.copy_(init)
        self.before = self.buf.clone()
        self.lead, self.shape, self.ld = lead, (rows, cols), ld

    @classmethod
    def _inner(cls, buf, lead, rows, cols, ld):
        return buf[lead:].view(rows + 2 * cls.GUARD, ld)[cls.GUARD:cls.GUARD + rows, :cols]

    def check(self, expected=None, what=""):
        want = self.before.clone()
        if expected is not None:
            rows, cols = self.shape
            self._inner(want, self.lead, rows, cols, self.ld).copy_(expected.to(want.device).reshape(rows, cols))
        torch.cuda.synchronize()
        if not torch.equal(bits(self.buf), bits(want)):
            inside = same(self.view, self._inner(want, self.lead, *self.shape, self.ld))
            raise AssertionError(f"{what}: " + ("a write outside the output view" if inside else "wrong values"))


def t2n(t):
    return t.detach().cpu().numpy()


def n2t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def refuses(fn, *guards):
    """fn() raises MapfedError and every guarded buffer is untouched (nothing was launched)."""
    with pytest.raises(MapfedError):
        fn()
    for gd in guards:
        gd.check(None, "a refused call wrote")


# ------------------------------------------------------------------------------------------------- im2col
IM2COL_SHAPES = [(3, 32, 16), (2, 24, 8), (1, 224, 16)]


def im2col_image(B, R, P, fp32):
    g = gen(B, R, P, fp32)
    if not fp32:
        return rand16(g, B, 3, R, R)
    img = rand32(g, B, 3, R, R)
    # exact fp16 ties (to even: down, up), the overflow threshold 65520 and its neighbours, fp16 subnormals and the
    # tie between 0 and the smallest of them
    special = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2048 + 1, 2048 + 3, 65504.0, 65519.99, 65520.0,
               70000.0, -65520.0, 1e38, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -20),
               5.7e-8, 0.0, -0.0]
    flat = img.view(-1)
    flat[:len(special)] = torch.tensor(special)
    flat[-len(special):] = torch.tensor(special)
    return img


def im2col_ref(img, P):
    B, _, R, _ = img.shape
    G = R // P
    return img.half().view(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * P * P)


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,R,P", IM2COL_SHAPES)
def test_im2col_patch(dev, B, R, P, fp32):
    """Exact: out = img.half() laid out [B, G, G, 3, P, P] (torch's CPU cast: ties to even, above 65520 to inf,
    subnormals kept)."""
    img = im2col_image(B, R, P, fp32)
    ref = im2col_ref(img, P)
    if fp32:
        assert torch.isinf(ref).sum().item() >= 6 and (ref.abs() < 2.0 ** -14).logical_and(ref != 0).any()
    out = Guarded(dev, ref.shape[0], ref.shape[1])
    ops.im2col_patch(img.to(dev), out.view, P)
    out.check(ref, f"im2col {B, R, P}")


# ------------------------------------------------------------------------------------------- the assemblers
def vision_case(B, G2, n_ctx, D):
    g = gen(B, G2, n_ctx, D)
    return dict(patch=rand16(g, B * G2, D), cls=rand32(g, D), pos=rand32(g, G2 + 1, D),
                sc=rand16(g, n_ctx, D) if n_ctx else None)


@pytest.mark.parametrize("D", [4, 64, 260])
@pytest.mark.parametrize("n_ctx", [0, 2, 4])
def test_vision_assemble(dev, n_ctx, D):
    """Exact against torch's CPU fp16 ops: fp16(fp16(cls) + fp16(pos[0])) | fp16(patch + fp16(pos[1 + p])) |
    shared_ctx."""
    B, G2 = 3, 4
    c = vision_case(B, G2, n_ctx, D)
    L = G2 + 1 + n_ctx
    top = torch.cat([c["cls"].half().expand(B, 1, D), c["patch"].view(B, G2, D)], 1) + c["pos"].half()
    ref = torch.cat([top, c["sc"].expand(B, -1, -1)], 1) if n_ctx else top
    x = Guarded(dev, B * L, D)
    d = {k: (v.to(dev) if v is not None else None) for k, v in c.items()}
    ops.vision_assemble(d["patch"], d["cls"], d["pos"], d["sc"], x.view, B, G2, n_ctx, D)
    x.check(ref, f"vision_assemble n_ctx={n_ctx} D={D}")


@pytest.mark.parametrize("D", [4, 260])
@pytest.mark.parametrize("K", [1, 5])
def test_text_assemble(dev, K, D):
    """Exact against torch's CPU fp16 ops: fp16((prefix | ctx | suffix) + fp16(pos)), n_ctx in {0, 2, 4} and
    L in {n_ctx + 1 (no suffix), 8}."""
    for n_ctx, full in itertools.product([0, 2, 4], [False, True]):
        L = 8 if full else n_ctx + 1
        ns = L - 1 - n_ctx
        g = gen(K, D, n_ctx, L)
        prefix, pos = rand16(g, K, 1, D), rand32(g, L, D)
        ctx = rand16(g, n_ctx, D) if n_ctx else None
        suffix = rand16(g, K, ns, D) if ns else None
        parts = [prefix] + ([ctx.expand(K, -1, -1)] if n_ctx else []) + ([suffix] if ns else [])
        ref = torch.cat(parts, 1) + pos.half()
        x = Guarded(dev, K * L, D)
        on = lambda t: t.to(dev) if t is not None else None
        ops.text_assemble(on(prefix), on(ctx), on(suffix), on(pos), x.view, K, L, n_ctx, D)
        x.check(ref, f"text_assemble K={K} D={D} n_ctx={n_ctx} L={L}")


# ------------------------------------------------------------------------------------------- prompt inject
@pytest.mark.parametrize("D", [4, 260])
@pytest.mark.parametrize("N", [1, 3])
def test_prompt_inject_fwd(dev, N, D):
    """Exact: the injected rows equal prompt.half(); every other row of x, and the guard rows, keep the sentinel."""
    L = 5
    for nrows in (1, 2, L):
        for row0 in sorted({0, 1, L - nrows}):
            if row0 + nrows > L:
                continue
            prompt = rand32(gen(N, D, nrows, row0), nrows, D)
            x = Guarded(dev, N * L, D)
            ops.prompt_inject_fwd(x.view, prompt.to(dev), N, L, row0, nrows, D)
            want = torch.full((N, L, D), SENTINEL, dtype=F16)
            want[:, row0:row0 + nrows] = prompt.half()
            x.check(want, f"inject_fwd N={N} D={D} row0={row0} nrows={nrows}")


INJ_L = 6
INJ_N = (1, 15, 16, 17, 33)
INJ_D = (4, 252, 256, 260, 768)
# every (N, out dtype, accumulate) triple; D, nrows, row0 and zero_rows cycle through their values at coprime strides
INJ_CASES = [(N, INJ_D[(i + i // 5) % 5], (1, 2, 4)[i % 3], bool((i // 2) % 2), o16, acc, bool((i + i // 4) % 2))
             for i, (N, o16, acc) in enumerate(itertools.product(INJ_N, (False, True), (False, True)))]


def inject_bwd_case(N, D, nrows, last, o16, acc, zero):
    g = gen(N, D, nrows, last, o16, acc, zero)
    dx = rand16(g, N, INJ_L, D)
    prior = (rand16(g, nrows, D) if o16 else rand32(g, nrows, D)) if acc else None
    return dx, prior, (INJ_L - nrows if last else 0)


@pytest.mark.parametrize("N,D,nrows,last,o16,acc,zero", INJ_CASES)
def test_prompt_inject_bwd(dev, N, D, nrows, last, o16, acc, zero):
    """Restatement (E.inject_bwd_out: group g sums n = g, g + 16, ...; red[0] + .. + red[15]; fp16 out rounds once,
    accumulate adds r16(t) to the prior value), bit for bit; then fp64 within SUM_UNITS.  dx afterwards: the
    injected rows exact +0 iff zero_rows, everything else as it was."""
    dx, prior, row0 = inject_bwd_case(N, D, nrows, last, o16, acc, zero)
    rows = t2n(dx[:, row0:row0 + nrows])
    want = E.inject_bwd_out(rows, o16, None if prior is None else t2n(prior))
    gdx = Guarded(dev, N * INJ_L, D, init=dx.view(N * INJ_L, D))
    out = Guarded(dev, nrows, D, dtype=F16 if o16 else F32, init=prior)
    ops.prompt_inject_bwd(gdx.view, N, INJ_L, row0, nrows, D, out.view, accumulate=acc, zero_rows=zero)
    what = f"inject_bwd N={N} D={D} nrows={nrows} row0={row0} f16={o16} acc={acc} zero={zero}"
    out.check(n2t(want), what)
    after = dx.clone()
    if zero:
        after[:, row0:row0 + nrows] = 0.0
    gdx.check(after, what + " (dx)")
    r64 = rows.astype(np.float64)
    t64, scale = r64.sum(0), np.abs(r64).sum(0)
    extra = 0.0
    if prior is not None:
        p64 = t2n(prior).astype(np.float64)
        extra = 0.5 * E.ulp(t64, 11) if o16 else E.ulp(np.abs(p64) + scale, 24)  # r16(t) / the fp32 add
        t64, scale = t64 + p64, scale + np.abs(p64)
    print(what, "fp64:", round(E.check64(want, t64, scale, SUM_UNITS["inject"], extra, what), 3))


# ------------------------------------------------------------------------------------- seq_grow, seq_scatter
@pytest.mark.parametrize("D", [8, 72])
@pytest.mark.parametrize("N", [1, 3])
def test_seq_grow_and_bwd(dev, N, D):
    """Exact against torch.cat and slicing, ncap in {0, 1, 4} x n_ctx in {0, 2, Lp}; the dropped rows of dsrc are
    exact +0."""
    Lp = 9
    for ncap, n_ctx in itertools.product([0, 1, 4], [0, 2, Lp]):
        g = gen(N, D, ncap, n_ctx)
        L = Lp + ncap
        src, cap, prompt = rand16(g, N, Lp, D), rand16(g, ncap, D), rand32(g, n_ctx, D)
        want = torch.cat([src[:, :Lp - n_ctx], cap.expand(N, -1, -1), prompt.half().expand(N, -1, -1)], 1)
        dst = Guarded(dev, N * L, D)
        ops.seq_grow(src.view(N * Lp, D).to(dev), dst.view, cap.to(dev) if ncap else None, prompt.to(dev), N, Lp,
                     ncap, n_ctx, D)
        dst.check(want, f"seq_grow N={N} D={D} ncap={ncap} n_ctx={n_ctx}")
        ddst = rand16(g, N, L, D)
        wantb = torch.zeros(N, Lp, D, dtype=F16)
        wantb[:, :Lp - n_ctx] = ddst[:, :Lp - n_ctx]
        dsrc = Guarded(dev, N * Lp, D)
        ops.seq_grow_bwd(ddst.view(N * L, D).to(dev), dsrc.view, N, Lp, ncap, n_ctx, D)
        dsrc.check(wantb, f"seq_grow_bwd N={N} D={D} ncap={ncap} n_ctx={n_ctx}")


@pytest.mark.parametrize("N,L_live,L_full,C", [(1, 3, 3, 8), (1, 1, 4, 24), (2, 2, 5, 24), (3, 5, 5, 264)])
def test_seq_scatter_strided(dev, N, L_live, L_full, C):
    """Exact: a strided src (ld C + 8) into a strided dst (ld C + 16); dst's other rows and its pad columns keep the
    sentinel."""
    src = rand16(gen(N, L_live, L_full, C), N * L_live, C)
    wide = torch.full((N * L_live, C + 8), SENTINEL, dtype=F16)
    wide[:, :C] = src
    dst = Guarded(dev, N * L_full, C, pad=16)
    ops.seq_scatter(wide.to(dev)[:, :C], dst.view, N, L_live, L_full)
    want = torch.full((N, L_full, C), SENTINEL, dtype=F16)
    want[:, :L_live] = src.view(N, L_live, C)
    dst.check(want, "seq_scatter")


# ------------------------------------------------------------------------------------------- caption pool
CAPTION_VOCAB = 50
CAPTION_CASES = [(1, 1, 64), (3, 1, 260), (3, 3, 100), (3, 64, 260), (1, 65, 512), (3, 65, 64), (3, 77, 100),
                 (1, 77, 512), (3, 128, 512), (1, 128, 260), (1, 64, 100), (1, 3, 64)]


def caption_case(B, T, D):
    g = gen(B, T, D)
    table = 0.05 * torch.randn(CAPTION_VOCAB, D, generator=g)       # not fp16 values: the kernel casts each entry
    tok = torch.randint(0, CAPTION_VOCAB, (B, T), generator=g).to(torch.int32)
    tok[0, 0] = 0
    tok[-1, -1] = CAPTION_VOCAB - 1
    if T >= 3:
        tok[:, 1] = tok[:, 2]                                       # a repeated id
    return tok, table, torch.randn(D, generator=g).half()


def _caption_units(got, ref64):
    """Largest |got - ref64| in fp16 ulps of the fp64 value."""
    return float((np.abs(got.astype(np.float64) - ref64) / E.ulp(ref64, 11)).max())


@pytest.mark.parametrize("B,T,D", CAPTION_CASES)
def test_caption_pool(dev, B, T, D):
    """Restatement (E.caption_pool: scores from lane-strided partials and the xor butterfly, rounded to fp16; the
    softmax with fp32 expf; the pooled sum over the tokens in order of fp16-rounded products), bit for bit.  The
    kernel exposes neither scores nor probabilities, so they are asserted through the result: a score or a
    probability one fp16 ulp off moves every product of its token.  At T = 1 the probability is
    fp16(expf(0) / expf(0)) = 1 and the pooled row must equal fp16(table[id]) exactly.  The one operation that is
    not pinned by IEEE rounding is expf: elementwise_bounds.py moves it by one fp32 ulp either way and finds no
    pooled element of CAPTION_CASES changed (each probability is rounded to fp16 next), so numpy's expf serves.
    Then fp64 through the same fp16 rounding points, within CAPTION_ULPS fp16 ulps: elementwise_bounds.py,
    restatement against fp64, 0.500 in every case with T > 1 (the result's own rounding; no score differs from the
    rounded fp64 score), the same with expf moved; 4x margin.  MI355X: 0.500 in every case, no element differs from
    the restatement."""
    tok, table, w = caption_case(B, T, D)
    pooled = Guarded(dev, B, D)
    ops.caption_pool(tok.to(dev), table.to(dev), w.to(dev), pooled.view)
    pooled.check(pooled.view.clone(), "caption_pool")       # the guard rows only
    got = t2n(pooled.view)
    if T == 1:
        assert same(pooled.view.cpu(), table[tok[:, 0].long()].half())
        return
    want = E.caption_pool(t2n(tok), t2n(table), t2n(w))
    ref64 = E.caption_pool64(t2n(tok), t2n(table), t2n(w))
    u_r, u_64 = _caption_units(got, want.astype(np.float64)), _caption_units(got, ref64)
    print(f"caption_pool B={B} T={T} D={D}: {u_r:.3f} fp16 ulps from the restatement, {u_64:.3f} from fp64, "
          f"{(got != want).mean():.5f} of the elements differ from the restatement")
    assert u_64 <= CAPTION_ULPS
    assert same(pooled.view.cpu(), n2t(want))


def test_caption_pool_bad_ids(dev):
    """An id of -1 or vocab makes exactly its own row NaN; the other row is bit for bit the clean call's."""
    B, T, D = 3, 65, 100
    tok, table, w = caption_case(B, T, D)
    clean = Guarded(dev, B, D)
    ops.caption_pool(tok.to(dev), table.to(dev), w.to(dev), clean.view)
    bad = tok.clone()
    bad[0, 64] = -1
    bad[2, 0] = CAPTION_VOCAB
    pooled = Guarded(dev, B, D)
    ops.caption_pool(bad.to(dev), table.to(dev), w.to(dev), pooled.view)
    pooled.check(pooled.view.clone(), "caption_pool bad ids")
    assert torch.isnan(pooled.view[0]).all() and torch.isnan(pooled.view[2]).all()
    assert same(pooled.view[1], clean.view[1]) and torch.isfinite(clean.view).all()


# ---------------------------------------------------------------------------------------------- transpose
# (R, C, pad_in, pad_out, lead_in, lead_out)
_TR_VARIANTS = [(0, 0, 0, 0), (8, 8, 0, 0), (2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
TRANSPOSE_CASES = ([(R, C, 0, 0, 0, 0) for R, C in [(1, 1), (63, 65), (65, 63), (130, 200)]] +
                   [(R, C) + v for R, C in [(64, 64), (128, 192)] for v in _TR_VARIANTS])


@pytest.mark.parametrize("R,C,pad_in,pad_out,lead_in,lead_out", TRANSPOSE_CASES)
def test_transpose(dev, R, C, pad_in, pad_out, lead_in, lead_out):
    """Exact: out = in.t(); out's pad columns, guard rows and lead keep the sentinel."""
    a = rand16(gen(R, C, pad_in, lead_in), R, C)
    src = Guarded(dev, R, C, pad=pad_in, lead=lead_in, init=a)
    out = Guarded(dev, C, R, pad=pad_out, lead=lead_out)
    ops.transpose(src.view, out.view)
    out.check(a.t(), f"transpose {R, C, pad_in, pad_out, lead_in, lead_out}")
    src.check(a, "transpose wrote its input")


# ------------------------------------------------------------------------------------------------- colsum
COLSUM_R = (1, 15, 16, 17, 63, 64, 65, 130)
COLSUM_C = (4, 252, 256, 260)
# every (R, output kind); C, the pad and the 4-element lead cycle at coprime strides
COLSUM_CASES = [(R, COLSUM_C[(i + i // 4) % 4], (0, 4, 8)[i % 3], 4 * int(i % 5 in (1, 3)), kind)
                for i, (R, kind) in enumerate(itertools.product(COLSUM_R, ("f16", "f32", "none")))]


def colsum_case(R, C, pad, lead, kind):
    return rand16(gen(R, C, pad, lead, len(kind), ord(kind[1])), R, C)


@pytest.mark.parametrize("R,C,pad,lead,kind", COLSUM_CASES)
def test_colsum(dev, R, C, pad, lead, kind):
    """Restatement (E.colsum_partials: wave w sums its 16 rows in order, red[0] + .. + red[3]; E.col_reduce:
    col_reduce_kernel's grouping), bit for bit: the partials [blocks][C] in the workspace (the interface to
    mf_col_reduce_batch) in every case, and out (fp16 / fp32) where given; then fp64 within SUM_UNITS."""
    x = colsum_case(R, C, pad, lead, kind)
    xin = Guarded(dev, R, C, pad=pad, lead=lead, init=x)
    nb = (R + 63) // 64
    assert ops.colsum_ws_floats(R, C) == nb * C
    ws = Guarded(dev, nb, C, dtype=F32)
    out = None if kind == "none" else Guarded(dev, 1, C, dtype=F16 if kind == "f16" else F32)
    ops.colsum(xin.view, None if out is None else out.view.view(C), ws.view.view(-1))
    what = f"colsum R={R} C={C} pad={pad} lead={lead} {kind}"
    part = E.colsum_partials(t2n(x))
    ws.check(n2t(part), what + " partials")
    xin.check(x, what + " input")
    if out is not None:
        want = E.colsum(t2n(x), kind == "f16")
        out.check(n2t(want), what)
        x64 = t2n(x).astype(np.float64)
        print(what, "fp64:", round(E.check64(want, x64.sum(0), np.abs(x64).sum(0), SUM_UNITS["colsum"], 0.0, what), 3))


# ------------------------------------------------------------------------------------------ small linears
SL_O = (1, 15, 16, 17, 31, 32, 33, 48, 768)
SL_I = (1, 63, 64, 65, 512)
SL_M = (1, 2, 16)
# every (O, dtype); I, M, the bias, the absent output and accumulate_dx cycle at coprime strides.  absent: which of
# dX / dW / db is null (3: none)
SL_CASES = [(f16, SL_M[(i + i // 3) % 3], SL_I[(i + i // 5) % 5], O, i % 2 == 0, (i + i // 4) % 4, (i // 2) % 2 == 0)
            for i, (O, f16) in enumerate(itertools.product(SL_O, (False, True)))]
SL_CASES += [(False, 16, 512, 768, True, 3, True), (True, 16, 65, 48, False, 3, True),
             (False, 2, 63, 48, True, 3, False)]


def small_linear_case(f16, M, I, O, bias, absent, acc):
    g = gen(f16, M, I, O, bias, absent, acc)
    # exponents -8 .. 0: an O = 768 dot product of such fp16 operands stays far below 65504
    mk = (lambda *s: rand16(g, *s, hi=1)) if f16 else (lambda *s: rand32(g, *s, hi=1))
    return dict(X=mk(M, I), W=mk(O, I), b=mk(O) if bias else None, dY=mk(M, O), dX0=mk(M, I) if acc else None)


def _mm_scale(a, b):
    return np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64))


@pytest.mark.parametrize("f16,M,I,O,bias,absent,acc", SL_CASES)
def test_small_linear(dev, f16, M, I, O, bias, absent, acc):
    """Restatement, bit for bit: Y (lane-strided partials, butterfly, + bias, one rounding), dX (E.small_linear_dx:
    two accumulators per group while o + 16 < O, the tail into the first, the 16 groups in order; accumulate adds
    the rounded term to the prior value), dW and db (serial over m); then fp64 within SUM_UNITS.  A null dX, dW or
    db leaves the others as they are; db is written by the dW kernel, so a null dW leaves db untouched.  X, W and
    dY sit in guarded allocations too and are unchanged afterwards."""
    c = small_linear_case(f16, M, I, O, bias, absent, acc)
    dt = F16 if f16 else F32
    gin = {k: Guarded(dev, v.shape[0], v.shape[1], dtype=dt, init=v) for k, v in c.items() if k in ("X", "W", "dY")}
    d = dict({k: g.view for k, g in gin.items()}, b=c["b"].to(dev) if bias else None)
    n = {k: (t2n(v) if v is not None else None) for k, v in c.items()}
    what = f"small_linear f16={f16} M={M} I={I} O={O} bias={bias} absent={absent} acc={acc}"
    Y = Guarded(dev, M, O, dtype=dt)
    ops.small_linear_fwd(d["X"], d["W"], d["b"], Y.view)
    wantY = E.small_linear_fwd(n["X"], n["W"], n["b"])
    Y.check(n2t(wantY), what + " Y")
    dX = Guarded(dev, M, I, dtype=dt, init=c["dX0"])
    dW = Guarded(dev, O, I, dtype=dt)
    db = Guarded(dev, 1, O, dtype=dt)
    ops.small_linear_bwd(d["dY"], d["X"], d["W"], None if absent == 0 else dX.view, None if absent == 1 else dW.view,
                         None if absent == 2 else db.view.view(O), accumulate_dx=acc)
    wantdX = E.small_linear_dx(n["dY"], n["W"], n["dX0"])
    wantdW, wantdb = E.small_linear_dw_db(n["dY"], n["X"])
    dX.check(None if absent == 0 else n2t(wantdX), what + " dX")
    dW.check(None if absent == 1 else n2t(wantdW), what + " dW")
    db.check(None if absent in (1, 2) else n2t(wantdb), what + " db")
    for k, g in gin.items():
        g.check(c[k], what + f" input {k}")
    X64, W64, dY64 = (n[k].astype(np.float64) for k in ("X", "W", "dY"))
    # fp32 operands: each product is rounded too, one more ulp of the scale at most
    y64, ys = X64 @ W64.T, _mm_scale(n["X"], n["W"].T)
    if bias:
        y64, ys = y64 + n["b"].astype(np.float64), ys + np.abs(n["b"].astype(np.float64))
    worst = [E.check64(wantY, y64, ys, SUM_UNITS["linear"], 0.0, what + " Y")]
    dx64, dxs, extra = dY64 @ W64, _mm_scale(n["dY"], n["W"]), 0.0
    if acc:
        p64 = n["dX0"].astype(np.float64)
        extra = 0.5 * E.ulp(dx64, 11) if f16 else E.ulp(np.abs(p64) + dxs, 24)  # the rounded term / the fp32 add
        dx64, dxs = dx64 + p64, dxs + np.abs(p64)
    worst.append(E.check64(wantdX, dx64, dxs, SUM_UNITS["linear"], extra, what + " dX"))
    worst.append(E.check64(wantdW, dY64.T @ X64, _mm_scale(n["dY"].T, n["X"]), SUM_UNITS["linear"], 0.0, what + " dW"))
    worst.append(E.check64(wantdb, dY64.sum(0), np.abs(dY64).sum(0), SUM_UNITS["linear"], 0.0, what + " db"))
    print(what, "fp64:", [round(v, 3) for v in worst])


def test_small_linear_batch_ragged(dev):
    """One batch whose entries differ in M (1, 2, 16), I (63, 512), O (17, 768) and dtype, so max_m, max_i, max_oi
    and max_mo exceed most entries' own sizes; one entry without dX, one without dW / db, one without bias.  Exact:
    every output equals the one-at-a-time kernels' bit for bit; absent outputs and every guard band are untouched."""
    specs = [(True, 1, 63, 17, True, 3, True), (False, 2, 512, 768, True, 0, False),
             (False, 16, 63, 768, True, 1, True), (True, 16, 512, 17, False, 3, False)]
    ents, singles, guards = [], [], []
    for f16, M, I, O, bias, absent, acc in specs:
        c = small_linear_case(f16, M, I, O, bias, absent, acc)
        dt = F16 if f16 else F32
        d = {k: (v.to(dev) if v is not None else None) for k, v in c.items()}
        pair = []
        for _ in range(2):
            pair.append(dict(Y=Guarded(dev, M, O, dtype=dt), dX=Guarded(dev, M, I, dtype=dt, init=c["dX0"]),
                             dW=Guarded(dev, O, I, dtype=dt), db=Guarded(dev, 1, O, dtype=dt)))
        one, bat = pair
        ops.small_linear_fwd(d["X"], d["W"], d["b"], one["Y"].view)
        ops.small_linear_bwd(d["dY"], d["X"], d["W"], None if absent == 0 else one["dX"].view,
                             None if absent == 1 else one["dW"].view, None if absent == 1 else one["db"].view.view(O),
                             accumulate_dx=acc)
        ents.append(dict(X=d["X"], W=d["W"], b=d["b"], Y=bat["Y"].view, dY=d["dY"],
                         dX=None if absent == 0 else bat["dX"].view, dW=None if absent == 1 else bat["dW"].view,
                         db=None if absent == 1 else bat["db"].view.view(O), acc_dx=acc))
        singles.append(one)
        guards.append(bat)
    batch = ops.SmallLinearBatch(dev, ents)
    assert (batch.max_m, batch.max_i, batch.max_oi, batch.max_mo) == (16, 512, 768 * 512, 16 * 768)
    batch.fwd()
    batch.bwd()
    torch.cuda.synchronize()
    for k, ((f16, M, I, O, bias, absent, acc), one, bat) in enumerate(zip(specs, singles, guards)):
        for key in ("Y", "dX", "dW", "db"):
            untouched = (key == "dX" and absent == 0) or (key in ("dW", "db") and absent == 1)
            assert torch.equal(bits(bat[key].buf), bits(one[key].buf)), (k, key)
            if untouched:
                bat[key].check(None, f"entry {k} {key}")
            else:
                assert not torch.equal(bits(bat[key].buf), bits(bat[key].before)), (k, key)


# ------------------------------------------------------------------------------------------------- argmax
ARGMAX_B = (1, 15, 16, 17, 100)
ARGMAX_K = (1, 63, 64, 65, 1000)


def argmax_rows(B, K):
    """fp16 logits [B, K]: row r carries pattern (r + shift) % 9 (shift: K's position in ARGMAX_K, so B = 1 meets five
    of them), where K has room for it: 0 a tie inside one lane (k, k + 64); 1 a tie across lanes (k = 5, 70); 2 a tie
    whose larger index sits in the lower lane (k = 70 in lane 6, k = 10 in lane 10; K = 65: k = 64 in lane 0, k = 3);
    3 two NaNs (the higher index in the lower lane at K = 1000) beside a larger finite value; 4 all NaN; 5 +inf at
    the end among finite values; 6 all -inf; 7 -0.0 before +0.0 above negative values; 8 plain."""
    g = gen(B, K)
    x = torch.randn(B, K, generator=g).half()
    nan, inf = float("nan"), float("inf")
    for r in range(B):
        p = (r + ARGMAX_K.index(K)) % 9
        if p == 0 and K > 64:
            k = 5 if K > 69 else 0
            x[r, k] = x[r, k + 64] = 9.0
        elif p == 1 and K > 9:
            x[r, 5] = x[r, 70 if K > 70 else 9] = 9.0
        elif p == 2 and K > 64:
            hi, lo = (70, 10) if K > 70 else (64, 3)
            x[r, hi] = x[r, lo] = 9.0
        elif p == 3 and K > 7:
            a, b = (130, 897) if K > 900 else (3, 7)   # 130 is lane 2's, 897 lane 1's
            x[r, a] = x[r, b] = nan
            x[r, 1] = 30.0
        elif p == 4:
            x[r] = nan
        elif p == 5:
            x[r, K - 1] = inf
        elif p == 6:
            x[r] = -inf
        elif p == 7 and K > 4:
            x[r] = -x[r].abs() - 1
            x[r, 2], x[r, 4] = -0.0, 0.0
    return x


@pytest.mark.parametrize("K", ARGMAX_K)
@pytest.mark.parametrize("B", ARGMAX_B)
def test_argmax_correct_edges(dev, B, K):
    """Exact: pred equals torch.argmax of the CPU float copy (first maximum, NaN the maximum); acc accumulates
    [hits, B] over two calls; each of label, pred, acc may be null on its own."""
    x = argmax_rows(B, K)
    ref = x.float().argmax(1)
    if K == 1000 and B >= 15:
        shift = ARGMAX_K.index(K)
        rows = {p: (p - shift) % 9 for p in range(9)}
        assert [ref[rows[p]].item() for p in (0, 1, 2, 3, 4, 5, 6, 7)] == [5, 5, 10, 130, 0, 999, 0, 2]
    g = gen(B, K, 1)
    label = torch.randint(0, K, (B,), generator=g)
    label[::2] = ref[::2]
    hits = (ref == label).sum().item()
    xd, ld = x.to(dev), label.to(dev)
    pred = Guarded(dev, 1, B, dtype=torch.int64)
    acc = Guarded(dev, 1, 2, dtype=F32, init=torch.zeros(1, 2))
    for n in (1, 2):
        ops.argmax_correct(xd, ld, pred.view.view(B), acc.view.view(2))
        pred.check(ref, f"argmax B={B} K={K}")
        acc.check(torch.tensor([[n * hits, n * B]], dtype=F32), f"argmax acc B={B} K={K}")
    # label null: no hits are counted; pred null; acc null
    pred2 = Guarded(dev, 1, B, dtype=torch.int64)
    ops.argmax_correct(xd, None, pred2.view.view(B), acc.view.view(2))
    pred2.check(ref, "argmax without labels")
    acc.check(torch.tensor([[2 * hits, 3 * B]], dtype=F32), "argmax acc without labels")
    ops.argmax_correct(xd, ld, None, acc.view.view(2))
    acc.check(torch.tensor([[3 * hits, 4 * B]], dtype=F32), "argmax acc without pred")
    pred3 = Guarded(dev, 1, B, dtype=torch.int64)
    ops.argmax_correct(xd, ld, pred3.view.view(B), None)
    pred3.check(ref, "argmax without acc")
    acc.check(torch.tensor([[3 * hits, 4 * B]], dtype=F32), "argmax wrote a null acc's neighbour")


# --------------------------------------------------------------------------------------------------- cast
def _cast(src, dst, n):
    call("mf_cast_f16_f32", ops._p(src), ops._p(dst), n, ops._s())


def test_cast_f16_f32_every_pattern(dev):
    """Exact: all 65 536 fp16 bit patterns against torch's CPU cast, NaNs by isnan, the rest by bits (subnormals and
    signed zeros included)."""
    src = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(F16)
    ref = src.float()
    out = Guarded(dev, 1, 65536, dtype=F32)
    _cast(src.to(dev), out.view, 65536)
    got = out.view.view(-1).cpu()
    nan = torch.isnan(ref)
    assert nan.sum().item() == 2 * 1023 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(bits(got)[~nan], bits(ref)[~nan])
    out.check(got, "cast")


@pytest.mark.parametrize("n", [1, 255, 257])
def test_cast_f16_f32_ragged(dev, n):
    src = rand16(gen(n), n)
    out = Guarded(dev, 1, n, dtype=F32)
    _cast(src.to(dev), out.view, n)
    out.check(src.float(), f"cast n={n}")


# ----------------------------------------------------------------------------------------- refused arguments
def _z(dev, *shape, dtype=F16):
    return torch.zeros(*shape, dtype=dtype, device=dev)


def test_refused_im2col_assemble(dev):
    """mf_im2col_patch: R % P, P % 8, a misaligned image or output.  The assemblers: D % 4, an fp16 operand that is
    not 8-byte aligned.  Nothing is launched: the outputs keep the sentinel."""
    out = Guarded(dev, 64, 768)
    img = _z(dev, 2 * 3 * 32 * 32 + 8, dtype=F32)
    raw = lambda img_p, out_p, R, P: call("mf_im2col_patch", img_p, 1, out_p, 2, R, P, ops._s())
    raw(ops._p(img), ops._p(out.view), 32, 16)
    out.check(out.view.clone(), "im2col")
    out = Guarded(dev, 64, 768)
    refuses(lambda: raw(ops._p(img), ops._p(out.view), 30, 16), out)                        # R % P
    refuses(lambda: raw(ops._p(img), ops._p(out.view), 24, 12), out)                        # P % 8 (3 P P % 8 == 0)
    refuses(lambda: raw(ops._p(img), ops._p(out.view), 24, 4), out)                         # P % 8
    refuses(lambda: raw(ops._p(img[1:]), ops._p(out.view), 32, 16), out)                    # img % 16
    refuses(lambda: raw(ops._p(img), ops._p(out.view.view(-1)[4:]), 32, 16), out)           # out % 16
    B, G2, n_ctx, D = 2, 4, 2, 8
    L = G2 + 1 + n_ctx
    x = Guarded(dev, B * L + 1, D)
    patch, cls, pos, sc = _z(dev, B * G2 * D + 8), _z(dev, D, dtype=F32), _z(dev, L * D, dtype=F32), _z(dev, n_ctx * D + 8)
    xv = x.view.view(-1)
    refuses(lambda: ops.vision_assemble(patch, cls, pos, sc, xv, B, G2, n_ctx, 6), x)       # D % 4
    refuses(lambda: ops.vision_assemble(patch[1:], cls, pos, sc, xv, B, G2, n_ctx, D), x)   # patch % 8
    refuses(lambda: ops.vision_assemble(patch, cls, pos, sc[2:], xv, B, G2, n_ctx, D), x)   # shared_ctx % 8
    refuses(lambda: ops.vision_assemble(patch, cls, pos, sc, xv[1:], B, G2, n_ctx, D), x)   # x % 8
    K, Lt = 2, 6
    xt = Guarded(dev, K * Lt + 1, D)
    tv = xt.view.view(-1)
    prefix, ctx, suffix = _z(dev, K * D + 8), _z(dev, n_ctx * D + 8), _z(dev, K * (Lt - 1 - n_ctx) * D + 8)
    post = _z(dev, Lt * D, dtype=F32)
    refuses(lambda: ops.text_assemble(prefix, ctx, suffix, post, tv, K, Lt, n_ctx, 6), xt)          # D % 4
    refuses(lambda: ops.text_assemble(prefix[1:], ctx, suffix, post, tv, K, Lt, n_ctx, D), xt)      # prefix % 8
    refuses(lambda: ops.text_assemble(prefix, ctx[3:], suffix, post, tv, K, Lt, n_ctx, D), xt)      # ctx % 8
    refuses(lambda: ops.text_assemble(prefix, ctx, suffix[2:], post, tv, K, Lt, n_ctx, D), xt)      # suffix % 8
    refuses(lambda: ops.text_assemble(prefix, ctx, suffix, post, tv[1:], K, Lt, n_ctx, D), xt)      # x % 8


def test_refused_inject_and_empty_work(dev):
    """mf_prompt_inject_fwd / _bwd: rows out of range, D % 4, a dx that is not 8-byte aligned are refused; N == 0 or
    nrows == 0 is empty work (returns 0, launches nothing).  The accepted form runs first."""
    N, L, D = 2, 5, 8
    x = Guarded(dev, N * L + 1, D)
    out = Guarded(dev, 2, D, dtype=F32)
    xv = x.view.view(-1)
    prompt = _z(dev, 2 * D, dtype=F32)
    ops.prompt_inject_bwd(xv, N, L, 3, 2, D, out.view, zero_rows=False)
    out.check(torch.full((2, D), 2 * SENTINEL), "inject_bwd of the sentinel")
    out = Guarded(dev, 2, D, dtype=F32)
    for row0, nrows in ((-1, 2), (4, 2), (0, L + 1)):
        refuses(lambda: ops.prompt_inject_fwd(xv, prompt, N, L, row0, nrows, D), x)
        refuses(lambda: ops.prompt_inject_bwd(xv, N, L, row0, nrows, D, out.view), x, out)
    refuses(lambda: ops.prompt_inject_bwd(xv, N, L, 3, 2, 6, out.view), x, out)             # D % 4
    refuses(lambda: ops.prompt_inject_bwd(xv[2:], N, L, 3, 2, D, out.view), x, out)         # dx % 8
    for n, nrows in ((0, 2), (N, 0), (0, 0)):
        ops.prompt_inject_fwd(xv, prompt, n, L, 3, nrows, D)
        ops.prompt_inject_bwd(xv, n, L, 3, nrows, D, out.view)
        x.check(None, "empty inject")
        out.check(None, "empty inject_bwd")


def test_refused_seq_grow_scatter(dev):
    """mf_seq_grow / _bwd: D % 8, n_ctx > Lp, n_ctx < 0, ncap < 0, an operand that is not 16-byte aligned.
    mf_seq_scatter: L_live of 0 or above L_full, C % 8, a leading dimension % 8 or below C, a misaligned operand."""
    N, Lp, ncap, n_ctx, D = 2, 6, 2, 2, 16
    L = Lp + ncap
    src, cap, prompt = _z(dev, N * Lp * D + 8), _z(dev, ncap * D + 8), _z(dev, Lp * D, dtype=F32)
    ddst = _z(dev, N * L * D + 8)
    dst, dsrc = Guarded(dev, N * L + 1, D), Guarded(dev, N * Lp + 1, D)
    dv, sv = dst.view.view(-1), dsrc.view.view(-1)
    grow = lambda s, d, c, ncap, n_ctx, D: call("mf_seq_grow", ops._p(s), ops._p(d), ops._p(c), ops._p(prompt), N,
                                                Lp, ncap, n_ctx, D, ops._s())
    bwd = lambda dd, ds, ncap, n_ctx, D: call("mf_seq_grow_bwd", ops._p(dd), ops._p(ds), N, Lp, ncap, n_ctx, D,
                                              ops._s())
    for bad in ((ncap, n_ctx, 12), (ncap, Lp + 1, D), (ncap, -1, D), (-1, n_ctx, D)):
        refuses(lambda: grow(src, dv, cap, *bad), dst)
        refuses(lambda: bwd(ddst, sv, *bad), dsrc)
    refuses(lambda: grow(src[4:], dv, cap, ncap, n_ctx, D), dst)                            # src % 16
    refuses(lambda: grow(src, dv[4:], cap, ncap, n_ctx, D), dst)                            # dst % 16
    refuses(lambda: grow(src, dv, cap[1:], ncap, n_ctx, D), dst)                            # cap % 16
    refuses(lambda: bwd(ddst[4:], sv, ncap, n_ctx, D), dsrc)                                # ddst % 16
    refuses(lambda: bwd(ddst, sv[2:], ncap, n_ctx, D), dsrc)                                # dsrc % 16
    grow(src, dv, cap, ncap, n_ctx, D)                                                      # the accepted form
    bwd(ddst, sv, ncap, n_ctx, D)
    torch.cuda.synchronize()
    assert (dst.view[:N * L] == 0).all() and (dsrc.view[:N * Lp] == 0).all()
    C = 16
    s2 = _z(dev, 4 * 3 * (C + 8) + 8)
    d2 = Guarded(dev, 4 * 5 + 1, C + 8)
    d2v = d2.view.view(-1)
    scat = lambda s, ld_s, d, ld_d, L_live, L_full, C: call("mf_seq_scatter", ops._p(s), ld_s, ops._p(d), ld_d, 4,
                                                             L_live, L_full, C, ops._s())
    for bad in ((s2, C, d2v, C, 0, 5, C), (s2, C, d2v, C, 6, 5, C), (s2, C, d2v, C, 3, 5, 12),
                (s2, C + 4, d2v, C, 3, 5, C), (s2, C, d2v, C + 4, 3, 5, C), (s2, 8, d2v, C, 3, 5, C),
                (s2, C, d2v, 8, 3, 5, C), (s2[4:], C, d2v, C, 3, 5, C), (s2, C, d2v[4:], C, 3, 5, C)):
        refuses(lambda: scat(*bad), d2)


def test_refused_caption_transpose_colsum(dev):
    """mf_caption_pool: T of 0 or 129, vocab <= 0.  mf_transpose_f16: ld_in < C, ld_out < R.  mf_colsum_f16 and
    mf_colsum_f16_live: C % 4, ld % 4, ld < C, a null workspace, an input that is not 8-byte aligned, a workspace
    that is not 16-byte aligned."""
    B, D, vocab = 2, 64, 10
    tok = torch.zeros(B * 129, dtype=torch.int32, device=dev)
    table, w = _z(dev, vocab * D, dtype=F32), _z(dev, D)
    pooled = Guarded(dev, B, D)
    pool = lambda T, vocab: call("mf_caption_pool", ops._p(tok), B, T, ops._p(table), vocab, ops._p(w), D,
                                 ops._p(pooled.view), ops._s())
    for bad in ((0, vocab), (129, vocab), (-1, vocab), (4, 0), (4, -3)):
        refuses(lambda: pool(*bad), pooled)
    R, C = 20, 12
    a = _z(dev, R * C)
    out = Guarded(dev, C, R)
    tr = lambda ld_in, ld_out: call("mf_transpose_f16", ops._p(a), ld_in, ops._p(out.view), ld_out, R, C, ops._s())
    refuses(lambda: tr(C - 1, R), out)
    refuses(lambda: tr(C, R - 1), out)
    refuses(lambda: tr(0, R), out)
    x = _z(dev, R * (C + 4) + 8)
    ws, o = Guarded(dev, 1, C + 4, dtype=F32), Guarded(dev, 1, C + 4, dtype=F32)
    wv, ov = ws.view.view(-1), o.view.view(-1)
    cs = lambda x_, ld, C_, ws_: call("mf_colsum_f16", ops._p(x_), ld, R, C_, ops._p(ov), 0, ws_, ops._s())
    live = lambda x_, ld, C_, ws_: call("mf_colsum_f16_live", ops._p(x_), ld, R, C_, ops._p(ov), 0, ws_, 1, R,
                                        ops._s())
    for f in (cs, live):
        refuses(lambda: f(x, C, 10, ops._p(wv)), ws, o)                                     # C % 4
        refuses(lambda: f(x, C + 2, C, ops._p(wv)), ws, o)                                  # ld % 4
        refuses(lambda: f(x, C - 4, C, ops._p(wv)), ws, o)                                  # ld < C
        refuses(lambda: f(x, C, C, None), ws, o)                                            # null workspace
        refuses(lambda: f(x[2:], C, C, ops._p(wv)), ws, o)                                  # in % 8
        refuses(lambda: f(x, C, C, ops._p(wv[1:])), ws, o)                                  # workspace % 16
    f = None
    cs(x[4:], C + 4, C, ops._p(wv))                                                         # 8-byte aligned: accepted
    torch.cuda.synchronize()
    assert (ov[:C] == 0).all() and (wv[:C] == 0).all() and (ov[C:] == SENTINEL).all()
