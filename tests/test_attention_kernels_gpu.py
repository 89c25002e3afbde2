"""The attention kernels (csrc/attention.hip) on every dispatch path against fp64: out, the LSE and dQ / dK / dV.

Which (N, H, L, causal) reaches which kernel, read off the five entry points (tiles = ceil(L / 16),
LKP = 16 tiles, LP = 32 ceil(L / 32), splits = attn_qsplit(N H, L)):

mf_attention_fwd
  L <= 256, N H < 2048 or L <= 128     attn_fwd4_kernel<LKP, causal>, grid (N H, splits), ceil(tiles / splits) waves.
                                        LKP = 16 .. 256, both masks: all 32 run (CASE1: one L per tile count, the
                                        causal ones at tiles 1 .. 16).  splits at N H = 4: 1 (tiles <= 3), 2 (4, 5),
                                        3 (6, 7), 4 (>= 8); 1 at 768 heads of 77 rows (CASE3 text)
  L > 256 (non-causal only)            attn_fwd4_kernel<LKP, false, 512>, LKP = 272 .. 512: all 16 run (CASE1 tiles
                                        17 .. 32).  4 splits at N H = 4 (5 .. 8 waves, one tile per wave); 2 splits at
                                        384 / 385 heads (CASE3): 8 waves and the continuation loop
                                        (fwd4_tile<., ., V_WAIT = false>), with the XCD-pairing remap of the block ids
                                        at 384 heads (a multiple of 8) and without it at 385
  N H >= 2048 and 128 < L <= 256       attn_fwdp_kernel<LKP, causal>, LKP = 144 .. 256.  Run here: <144, true> (CASE3,
                                        2 048 heads of 129 rows); test_kernels_gpu runs <160, false> and
                                        <208, false>.  Not run at kernel level: the other 13 (a launch is >= 2 048
                                        heads, and the tile code is fwd4_tile<LKP, causal, false>, which every
                                        LKP <= 256 runs through the fused in-projection kernel or not at all -- see
                                        below).  The LKP <= 128 cases of the dispatch switch cannot be reached (L > 128)
mf_attention_fwd_rows                  attn_fwd4_kernel<LKP, causal>, grid (N H, 1), ceil(q_rows / 16) waves: <208,
                                        false> and <80, true> at q_rows 1 and 17 through strided views
                                        (test_kernels_gpu runs the same two contiguous)
mf_qkv_attention_fwd
  D = 768, non-causal, L 193 .. 208    qkv_attn_fwd_vision_kernel (qkv_attn_fwd_body<208, 224, 768, false, 3>):
                                        L = 193, 208 at N = 1, 2
  D = 512, causal, L 65 .. 80          qkv_attn_fwd_text_kernel (qkv_attn_fwd_body<80, 96, 512, true, 2>):
                                        L = 65, 80 at N = 1, 2
mf_attention_bwd
  LP <= 224                            attn_bwd_fused_kernel<LP, causal, 1>, LP = 32 .. 224, both masks: all 14 run
  224 < L <= 256                       attn_bwd_dot_kernel, attn_bwd_dkv_kernel<256, causal>,
                                        attn_bwd_dq_kernel<256, causal>: both masks run (tiles 15, 16; L = 225, 256)
                                        UNREACHABLE: attn_bwd_dkv_kernel / attn_bwd_dq_kernel<32 .. 224, both masks>,
                                        28 instantiations behind MF_ATTN_DISPATCH(LP, CALLB): LP <= 224 has taken the
                                        fused kernel before that switch
  L > 256 (non-causal only)            attn_bwd_dot_kernel, attn_bwd_dkv_kernel<LP, false>, attn_bwd_dq_kernel<LP,
                                        false>, LP = 288 .. 512: all 8 run; grid (N H, splits), 8 waves
mf_attention_bwd_rows                  attn_bwd_fused_kernel<LP, false, 1, true>, LP = 32 .. 224: <224> here through
                                        strided views (q_rows 1, 17); test_train_cls_rows_gpu runs <32>, <64>, <224>.
                                        Not run: <96>, <128>, <160>, <192> (the engine calls it at 199 rows)

Every comparison is against fp64 on the GPU from the fp16 inputs: S = Q K^T / 8 (-inf above the diagonal when
causal), lse = logsumexp(S), out = softmax(S) V and the fp64 autograd gradients of that expression, computed once
per case (_case) and never written to.  The bounds are not chosen: tests/diagnostics/attention_bounds.py restates the
kernels' rounding points in torch on the CPU, measures that restatement against fp64 on these very inputs, and shows
that six plausible kernel mistakes break the bounds.  Each bound below is 4 x the figure it printed (the margin
test_reduction_kernels_gpu.py gives another legal fp32 summation order; here: the MFMA accumulation order and the
hardware exp2 / log).  One of the six, D from the kernel's own fp32 O instead of the stored fp16 O, lands closer to
fp64 than the kernels do and passes every bound of the issue's cases; CASE8 (the backward handed -out) is there for it.
"""
import functools
from collections import namedtuple

import pytest
import torch

from federated_multi_modal_amd import ops
from test_kernels_gpu import ulp16

pytestmark = pytest.mark.gpu

SENTINEL = -7.25  # exact in fp16; no kernel output equals it by accident in a whole pad column

# ---------------------------------------------------------------------------------------------------- bounds
# Figures (see figures()):  lse      max |lse - lse64|
#                           lse_rel  max |lse - lse64| / max(1, |lse64|)
#                           out, dq, dk, dv   worst max(0, |x - x64| - ulp16(x64) / 2) / max |x64| of the head
# Each line: 4 x the worst figure attention_bounds.py printed for the group  # that figure | the MI355X's worst.
#
# Unit-scale inputs (q, k, v, dout ~ N(0, 1) rounded to fp16): CASE1, CASE2, CASE3, CASE6, CASE7 and CASE5 at 2^0.
BOUND_UNIT = dict(
    lse=4 * 9.31e-7,  # restatement 9.31e-7 | MI355X 9.92e-7
    out=4 * 2.38e-4,  # restatement 2.38e-4 | MI355X 2.38e-4
    dq=4 * 7.97e-4,  # restatement 7.97e-4 | MI355X 7.97e-4
    dk=4 * 6.33e-4,  # restatement 6.33e-4 | MI355X 6.33e-4
    dv=4 * 4.14e-4,  # restatement 4.14e-4 | MI355X 4.14e-4
)
# q and k scaled by 6 (CASE4): row maxima of S beyond 88, a nearly one-hot softmax.  The LSE is m / 8 + log(l) with m an
# fp32 sum of 64 products: every term's rounding error is 2^-24 of its own size, so the error is held relative to
# max(1, |lse64|) instead of absolutely.
BOUND_PEAKED = dict(
    lse_rel=4 * 5.36e-7,  # restatement 5.36e-7 | MI355X 8.94e-7
    out=4 * 9.18e-5,  # restatement 9.18e-5 | MI355X 9.18e-5
    dq=4 * 2.43e-3,  # restatement 2.43e-3 | MI355X 2.43e-3
    dk=4 * 5.61e-3,  # restatement 5.61e-3 | MI355X 5.97e-3
    dv=4 * 1.40e-4,  # restatement 1.40e-4 | MI355X 1.40e-4
)
# q and k scaled by 1 / 16 (CASE4): an almost uniform softmax.
BOUND_FLAT = dict(
    lse=4 * 4.95e-7,  # restatement 4.95e-7 | MI355X 7.14e-7
    out=4 * 2.13e-4,  # restatement 2.13e-4 | MI355X 2.13e-4
    dq=4 * 2.54e-4,  # restatement 2.54e-4 | MI355X 2.54e-4
    dk=4 * 2.34e-4,  # restatement 2.34e-4 | MI355X 2.19e-4
    dv=4 * 3.73e-4,  # restatement 3.73e-4 | MI355X 3.73e-4
)
# dout scaled by 2^-8, 2^-14, 2^-20 (CASE5; 2^0 is held to BOUND_UNIT): what rounding P and dS = P (dP - D) to fp16
# costs without loss scaling.  out and lse do not depend on dout and stay at BOUND_UNIT.
BOUND_SMALL = {
    -8: dict(dq=4 * 2.77e-4, dk=4 * 2.73e-4, dv=4 * 2.06e-4),  # MI355X 2.77e-4, 2.73e-4, 2.06e-4
    -14: dict(dq=4 * 3.00e-3, dk=4 * 2.35e-3, dv=4 * 1.52e-4),  # MI355X 3.00e-3, 2.34e-3, 1.52e-4
    -20: dict(dq=4 * 1.50e-1, dk=4 * 1.45e-1, dv=4 * 6.34e-5),  # MI355X 1.50e-1, 1.45e-1, 6.34e-5
}
# The backward given -out in place of the forward's out (CASE8): D = sum_d dO_d out_d must come from the buffer it is
# handed.  dv does not depend on D and is held to BOUND_UNIT's figure.
BOUND_GIVEN_OUT = dict(
    dq=4 * 2.45e-4,  # restatement 2.45e-4 | MI355X 2.43e-4
    dk=4 * 3.08e-4,  # restatement 3.08e-4 | MI355X 3.08e-4
    dv=4 * 2.26e-4,  # restatement 2.26e-4 | MI355X 2.26e-4
)

# ----------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "tag N L H causal qk_scale", defaults=(1.0,))


def _tile_len(t):
    """One L with ceil(L / 16) = t that is no multiple of 16 (the last key tile has masked keys)."""
    return 16 * (t - 1) + 1 + (7 * t) % 15


CASE1 = [Case(1, 2, _tile_len(t), 2, False) for t in range(1, 33)] + \
        [Case(1, 2, _tile_len(t), 2, True) for t in range(1, 17)]
_EDGE_BOTH = (1, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 224, 225, 256)
_EDGE_LONG = (257, 272, 273, 511, 512)
CASE2 = [Case(2, 2, L, 2, c) for c in (False, True) for L in _EDGE_BOTH] + [Case(2, 2, L, 2, False) for L in _EDGE_LONG]
CASE3_SPLIT = [Case(3, N, L, H, False) for L in (300, 455) for (N, H) in ((48, 8), (55, 7))]
CASE3_TEXT = Case(3, 96, 77, 8, True)
CASE3_PERSISTENT = Case(3, 256, 129, 8, True)
CASE4_PEAKED = [Case(4, 2, L, 2, False, 6.0) for L in (50, 199, 230, 300)] + \
               [Case(4, 2, L, 2, True, 6.0) for L in (50, 230)]
CASE4_FLAT = [Case(4, 2, 199, 2, False, 1.0 / 16)]
CASE5 = [Case(5, 2, 199, 2, False), Case(5, 2, 77, 2, True)]
CASE5_EXPONENTS = (0, -8, -14, -20)
CASE6 = [Case(6, 3, 199, 2, False), Case(6, 3, 77, 2, True), Case(6, 3, 300, 2, False)]
CASE8 = [Case(8, 2, 199, 2, False), Case(8, 2, 77, 2, True), Case(8, 2, 240, 2, False), Case(8, 2, 300, 2, False)]
CASE7 = [(N, L, 12, False) for L in (193, 208) for N in (1, 2)] + [(N, L, 8, True) for L in (65, 80) for N in (1, 2)]


def _id(c):
    return f"N{c.N}-H{c.H}-L{c.L}-{'causal' if c.causal else 'full'}" + (f"-x{c.qk_scale:g}" if c.qk_scale != 1 else "")


def host_inputs(c):
    """qkv [N L, 3 D] and dout [N L, D] of a case, fp16 on the host (the diagnostic reads the same tensors)."""
    D = 64 * c.H
    g = torch.Generator().manual_seed(c.tag * 10 ** 8 + c.N * 10 ** 5 + c.L * 100 + 2 * c.H + int(c.causal))
    qkv = torch.randn(c.N * c.L, 3 * D, generator=g)
    qkv[:, :2 * D] *= c.qk_scale
    dout = torch.randn(c.N * c.L, D, generator=g)
    return qkv.half(), dout.half()


def host_inputs_fused(N, L, H):
    """x, W_in, b_in of a CASE7 shape: x has exactly N L rows."""
    D = 64 * H
    g = torch.Generator().manual_seed(7 * 10 ** 8 + N * 10 ** 5 + L * 100 + H)
    x = torch.randn(N * L, D, generator=g).half()
    w = (torch.randn(3 * D, D, generator=g) * D ** -0.5).half()
    b = (torch.randn(3 * D, generator=g) * 0.02).half()
    return x, w, b


def heads(t, N, L, H):
    """[N L, k H 64] (any leading dimension) -> k tensors [N, H, L, 64]."""
    k = t.shape[1] // (64 * H)
    return t.view(N, L, k, H, 64).permute(2, 0, 3, 1, 4).unbind(0)


def ref64(qkv, dout, N, L, H, causal):
    """out, lse (and dq, dk, dv when dout is given) in fp64 from the fp16 inputs, on their device."""
    q, k, v = (t.double().requires_grad_(dout is not None) for t in heads(qkv, N, L, H))
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    lse = torch.logsumexp(s, -1)
    out = torch.softmax(s, -1) @ v
    ref = dict(out=out.detach(), lse=lse.detach())
    if dout is not None:
        out.backward(heads(dout, N, L, H)[0].double())
        ref.update(dq=q.grad, dk=k.grad, dv=v.grad)
    return ref


def ref64_given_out(qkv, dout, out_given, N, L, H, causal):
    """dq, dk, dv in fp64 of the backward's own formula with D taken from out_given [N L, D] instead of softmax(S) V:
    dS = P (dP - D), D = sum_d dO_d out_given_d; dq = dS K / 8, dk = dS^T Q / 8, dv = P^T dO."""
    q, k, v = (t.double() for t in heads(qkv, N, L, H))
    do, og = heads(dout, N, L, H)[0].double(), heads(out_given, N, L, H)[0].double()
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    ds = p * (do @ v.transpose(-1, -2) - (do * og).sum(-1, keepdim=True))
    return dict(dq=ds @ k * 0.125, dk=ds.transpose(-1, -2) @ q * 0.125, dv=p.transpose(-1, -2) @ do)


def lse64(qkv, N, L, H, causal, chunk=8):
    """The fp64 LSE of every head [N, H, L], a few sequences at a time."""
    parts = []
    for s0 in range(0, N, chunk):
        n = min(chunk, N - s0)
        parts.append(ref64(qkv[s0 * L:(s0 + n) * L], None, n, L, H, causal)["lse"])
    return torch.cat(parts)


def as_heads(out, lse, dqkv, N, L, H):
    """Kernel outputs in the reference's layout."""
    got = {}
    if out is not None:
        got.update(out=heads(out, N, L, H)[0], lse=lse.view(N, H, -1)[:, :, :L])
    if dqkv is not None:
        got["dq"], got["dk"], got["dv"] = heads(dqkv, N, L, H)
    return got


def figures(got, ref):
    """The error figures the bounds are stated in.  A head whose fp64 result is exactly zero (dq and dk at L = 1: a
    one-key softmax has no gradient) has no unit of its own: it is left out of the figure and its largest |value| is
    reported as <name>_zero."""
    f = {}
    if "lse" in got:
        e = (got["lse"].double() - ref["lse"]).abs()
        f["lse"] = e.max().item()
        f["lse_rel"] = (e / ref["lse"].abs().clamp_min(1.0)).max().item()
    for k in ("out", "dq", "dk", "dv"):
        if k not in got:
            continue
        x64 = ref[k]
        x = got[k].double()
        d = ((x - x64).abs() - 0.5 * ulp16(x64).double()).clamp_min(0.0)
        top = x64.abs().amax(dim=(-2, -1), keepdim=True)
        live = (top > 0).expand_as(d)
        zero = torch.zeros((), dtype=d.dtype, device=d.device)
        f[k] = torch.where(live, d / top.clamp_min(1e-300), zero).max().item()
        f[k + "_zero"] = torch.where(live, zero, x.abs()).max().item()
    return f


def scaled_ref(ref, e):
    """The reference for dout 2^e: the gradients are linear in dout and the scaling is exact in fp64."""
    r = dict(ref)
    for k in ("dq", "dk", "dv"):
        r[k] = ref[k] * 2.0 ** e
    return r


def check(got, ref, bound, what, zero_tol=0.0):
    f = figures(got, ref)
    print(f"{what}: " + "  ".join(f"{k} {f[k]:.3e} (bound {bound[k]:.3e})" for k in bound))
    for k, t in got.items():
        assert torch.isfinite(t).all(), f"{what}: {k} has a NaN or an Inf"
    for k in bound:
        assert f[k] <= bound[k], f"{what}: {k} {f[k]:.3e} beyond {bound[k]:.3e}"
    for k in ("dq", "dk", "dv"):
        if k in got:
            assert f[k + "_zero"] <= zero_tol, f"{what}: {k} of a zero-gradient head {f[k + '_zero']:.3e}"
    return f


def zero_head_tol(qkv, dout, N, L, H):
    """dq and dk of a one-key softmax are zero.  The kernel's dS = P (dP - D) has dP and D as two fp32 sums of the
    same 64 exact products dO_d v_d in different orders, so |dP - D| <= 2 * 64 * 2^-24 * sum |dO_d v_d|; dq = dS k / 8
    and dk = dS q / 8, plus one fp16 subnormal step for the roundings."""
    q, k, v = heads(qkv, N, L, H)
    do = heads(dout, N, L, H)[0]
    s = (do.double().abs() * v.double().abs()).sum(-1).max().item()
    return 128 * 2.0 ** -24 * s * max(q.abs().max().item(), k.abs().max().item()) / 8 + 2.0 ** -24


def run(qkv, dout, N, L, H, causal):
    """Forward, then the backward on the forward's own out and lse, as the engine does."""
    out, lse = ops.attention_fwd(qkv, N, L, H, causal)
    dqkv = ops.attention_bwd(qkv, out, dout, lse, N, L, H, causal)
    return out, lse, dqkv


@functools.lru_cache(maxsize=None)
def _case(c):
    """Inputs of a small case on the GPU and their fp64 reference: computed once, never written to."""
    dev = torch.device("cuda:0")
    qkv, dout = (t.to(dev) for t in host_inputs(c))
    return qkv, dout, ref64(qkv, dout, c.N, c.L, c.H, c.causal)


def _check_causal_row0(c, qkv, out, lse):
    """Row 0 under the causal mask attends key 0 only: out = v[0] exactly (P = 1, l = 1), lse = q0 . k0 / 8 (an fp32
    sum of 64 exact products: within 64 * 2^-24 of sum |q0_d k0_d| / 8 of the fp64 value)."""
    q, k, v = heads(qkv, c.N, c.L, c.H)
    assert torch.equal(heads(out, c.N, c.L, c.H)[0][:, :, 0], v[:, :, 0]), "causal row 0 of out is not v[0]"
    prod = q[:, :, 0].double() * k[:, :, 0].double()
    err = (lse.view(c.N, c.H, -1)[:, :, 0].double() - prod.sum(-1) * 0.125).abs()
    assert (err <= 64 * 2.0 ** -24 * prod.abs().sum(-1) * 0.125).all(), "causal lse[0] is not q0 . k0 / 8"


# ------------------------------------------------------------------------------------- 1, 2: every instantiation
@pytest.mark.parametrize("c", CASE1 + CASE2, ids=lambda c: f"case{c.tag}-{_id(c)}")
def test_every_instantiation_and_edge_length(dev, c):
    """CASE1: one length per forward key-tile count (every attn_fwd4_kernel LKP, every reachable backward LP), the
    last key tile partly masked.  CASE2: L at LP, LP - 15, LP - 31 and 1, where padded rows are re-read (stage_rows),
    masked by LSE = +inf (backward) or absent.  out, lse, dq, dk, dv against fp64 at BOUND_UNIT."""
    qkv, dout, ref = _case(c)
    out, lse, dqkv = run(qkv, dout, c.N, c.L, c.H, c.causal)
    tol = zero_head_tol(qkv, dout, c.N, c.L, c.H) if c.L == 1 else 0.0
    check(as_heads(out, lse, dqkv, c.N, c.L, c.H), ref, BOUND_UNIT, _id(c), zero_tol=tol)
    if c.causal:
        _check_causal_row0(c, qkv, out, lse)


# ----------------------------------------------------------------------------------------- 3: head-count branches
def _check_edges_and_middle(c, qkv, dout, out, lse, dqkv, bound):
    """All of lse against fp64; out, dq, dk, dv on the first and the last two sequences; two sequences in the middle
    of the batch bit-identical to the same sequences run alone (another grid, another split count)."""
    N, L, H = c.N, c.L, c.H
    e = (lse.view(N, H, L).double() - lse64(qkv, N, L, H, c.causal)).abs().max().item()
    print(f"{_id(c)}: lse of all {N * H} heads {e:.3e} (bound {bound['lse']:.3e})")
    assert e <= bound["lse"]
    lse_v = lse.view(N * H, L)
    for s0 in (0, N - 2):
        rows = slice(s0 * L, (s0 + 2) * L)
        ref = ref64(qkv[rows], dout[rows], 2, L, H, c.causal)
        check(as_heads(out[rows], lse_v[s0 * H:(s0 + 2) * H], dqkv[rows], 2, L, H), ref, bound,
              f"{_id(c)} sequences {s0}, {s0 + 1}")
    s0 = N // 2 - 1
    rows = slice(s0 * L, (s0 + 2) * L)
    o2, l2, d2 = run(qkv[rows], dout[rows], 2, L, H, c.causal)
    assert torch.equal(out[rows], o2), "out depends on the grid"
    assert torch.equal(lse_v[s0 * H:(s0 + 2) * H], l2.view(2 * H, L)), "lse depends on the grid"
    assert torch.equal(dqkv[rows].view(torch.int16), d2.view(torch.int16)), "dqkv depends on the grid"


@pytest.mark.parametrize("c", CASE3_SPLIT + [CASE3_TEXT], ids=_id)
def test_head_count_branches(dev, c):
    """384 heads (N = 48, H = 8) and 385 (N = 55, H = 7) of 300 and 455 rows: attn_qsplit gives 2 splits, so each
    8-wave workgroup of attn_fwd4_kernel<., false, 512> has more than 8 tiles and runs its continuation loop; 384 is
    a multiple of 8 and takes the XCD-pairing remap of the block ids, 385 does not.  The long backward runs on a
    (heads, 2) grid.  768 causal heads of 77 rows: one split."""
    qkv, dout = (t.to(dev) for t in host_inputs(c))
    out, lse, dqkv = run(qkv, dout, c.N, c.L, c.H, c.causal)
    _check_edges_and_middle(c, qkv, dout, out, lse, dqkv, BOUND_UNIT)


def test_persistent_causal_forward(dev):
    """2 048 causal heads of 129 rows: attn_fwdp_kernel<144, true>.  out and lse bit-identical to slices of 64
    sequences (512 heads: attn_fwd4_kernel<144, true>); the first two sequences, with the backward on them, against
    fp64."""
    c = CASE3_PERSISTENT
    N, L, H = c.N, c.L, c.H
    qkv, dout = (t.to(dev) for t in host_inputs(c))
    out, lse = ops.attention_fwd(qkv, N, L, H, True)
    lse_v = lse.view(N * H, L)
    for s0 in range(0, N, 64):
        rows = slice(s0 * L, (s0 + 64) * L)
        o_s, l_s = ops.attention_fwd(qkv[rows], 64, L, H, True)
        assert torch.equal(out[rows], o_s), f"out of sequences {s0}.."
        assert torch.equal(lse_v[s0 * H:(s0 + 64) * H], l_s.view(64 * H, L)), f"lse of sequences {s0}.."
    rows = slice(0, 2 * L)
    dqkv = ops.attention_bwd(qkv[rows], out[rows], dout[rows], lse_v[:2 * H].reshape(-1), 2, L, H, True)
    ref = ref64(qkv[rows], dout[rows], 2, L, H, True)
    check(as_heads(out[rows], lse_v[:2 * H], dqkv, 2, L, H), ref, BOUND_UNIT, _id(c))
    _check_causal_row0(Case(3, 2, L, H, True), qkv[rows], out[rows], lse_v[:2 * H])


# ------------------------------------------------------------------------------------ 4: peaked and flat softmax
@pytest.mark.parametrize("c", CASE4_PEAKED + CASE4_FLAT, ids=_id)
def test_peaked_and_flat_softmax(dev, c):
    """q and k times 6: row maxima of S pass 88 (exp overflows fp32 without the row-max subtraction) and other scores
    sit more than 88 below them; lse = m / 8 + log(l) and the backward's exp2(s c - lse log2e) cancel large terms.
    q and k times 1 / 16: an almost uniform softmax.  No NaN or Inf, every output within its group's bound."""
    qkv, dout, ref = _case(c)
    if c.qk_scale > 1:
        s = (heads(qkv, c.N, c.L, c.H)[0].double() @ heads(qkv, c.N, c.L, c.H)[1].double().transpose(-1, -2)) * 0.125
        assert s.max().item() > 88 and (s.amax(-1) - s.amin(-1)).max().item() > 88  # the case is what it claims
    out, lse, dqkv = run(qkv, dout, c.N, c.L, c.H, c.causal)
    check(as_heads(out, lse, dqkv, c.N, c.L, c.H), ref, BOUND_PEAKED if c.qk_scale > 1 else BOUND_FLAT, _id(c))


# --------------------------------------------------------------------------------------------- 5: small gradients
@pytest.mark.parametrize("e", CASE5_EXPONENTS)
@pytest.mark.parametrize("c", CASE5, ids=_id)
def test_small_gradients(dev, c, e):
    """The same dout times 2^e (exact in fp16 until it goes subnormal; the reference is then taken from the rounded
    dout the kernel sees): the engine has no loss scaling, and the
    backward rounds P and dS = P (dP - D) to fp16 before the dV / dK / dQ products.  The kernel stays within 4 x the
    restatement's error at every scale; DESIGN.md records what that error is."""
    qkv, dout, ref = _case(c)
    dout_e = (dout.float() * 2.0 ** e).half()
    out, lse, dqkv = run(qkv, dout_e, c.N, c.L, c.H, c.causal)
    bound = dict(BOUND_UNIT)
    if e:
        bound.update(BOUND_SMALL[e])
    exact = torch.equal(dout_e.double(), dout.double() * 2.0 ** e)  # false once elements go subnormal
    ref_e = scaled_ref(ref, e) if exact else ref64(qkv, dout_e, c.N, c.L, c.H, c.causal)
    check(as_heads(out, lse, dqkv, c.N, c.L, c.H), ref_e, bound, f"{_id(c)} dout 2^{e}")


@pytest.mark.parametrize("c", CASE8, ids=_id)
def test_backward_takes_d_from_the_out_it_is_given(dev, c):
    """Not one of the issue's cases: the mistake "D from the kernel's own fp32 O instead of the stored fp16 O" brings
    dq and dk *closer* to fp64 (attention_bounds.py: up to 10 x on the peaked cases), so no upper bound against the
    fp64 gradient can see it.  What can: hand the backward -out.  D = sum_d dO_d out_d must then flip its sign, and
    dq / dk follow the backward's formula with that D (ref64_given_out).  199 rows and 77 causal: the fused kernel's
    phase 0; 240 and 300 rows: attn_bwd_dot_kernel before the two-kernel and the long backward."""
    qkv, dout, _ = _case(c)
    out, lse = ops.attention_fwd(qkv, c.N, c.L, c.H, c.causal)
    given = -out
    dqkv = ops.attention_bwd(qkv, given, dout, lse, c.N, c.L, c.H, c.causal)
    ref = ref64_given_out(qkv, dout, given, c.N, c.L, c.H, c.causal)
    check(as_heads(None, None, dqkv, c.N, c.L, c.H), ref, BOUND_GIVEN_OUT, _id(c) + " -out")


# ----------------------------------------------------------------------------------------- 6: isolation, strides
def _padded(t, pad):
    """A copy of the 2-D tensor as a view of leading dimension cols + pad, pad columns holding SENTINEL."""
    rows, cols = t.shape
    full = torch.full((rows, cols + pad), SENTINEL, dtype=t.dtype, device=t.device)
    full[:, :cols] = t
    return full[:, :cols], full


def _pads_intact(full, cols):
    return bool((full[:, cols:] == SENTINEL).all())


@pytest.mark.parametrize("c", CASE6, ids=_id)
def test_sequence_isolated_from_its_neighbours(dev, c):
    """The middle sequence of three: out, lse and dqkv bit-identical whether its neighbours hold the generated data
    or +-60 000 in every element of qkv and dout.  Padded rows re-read the sequence's own last row (stage_rows) or are
    clamped to it, never the next sequence's."""
    N, L, H, D = c.N, c.L, c.H, 64 * c.H
    qkv, dout, ref = _case(c)
    out, lse, dqkv = run(qkv, dout, N, L, H, c.causal)
    check(as_heads(out, lse, dqkv, N, L, H), ref, BOUND_UNIT, _id(c))
    qkv2, dout2 = qkv.clone(), dout.clone()
    sign = torch.where(torch.arange(3 * D, device=dev) % 3 == 0, -1.0, 1.0).half()
    for t in (qkv2, dout2):
        t[:L] = 60000.0
        t[2 * L:] = 60000.0 * sign[:t.shape[1]]
    out2, lse2, dqkv2 = run(qkv2, dout2, N, L, H, c.causal)
    mid = slice(L, 2 * L)
    assert torch.equal(out[mid], out2[mid])
    assert torch.equal(lse.view(N, H, L)[1], lse2.view(N, H, L)[1])
    assert torch.equal(dqkv[mid].view(torch.int16), dqkv2[mid].view(torch.int16))


@pytest.mark.parametrize("c", CASE6, ids=_id)
def test_leading_dimensions(dev, c):
    """ld_qkv = 3 D + 8, ld_out = D + 4, ld_dout = D + 8, ld_dqkv = 3 D + 4, ld_lse = L + 3: bit-identical to the
    contiguous run, every pad column and pad LSE slot untouched."""
    N, L, H, D = c.N, c.L, c.H, 64 * c.H
    qkv, dout, _ = _case(c)
    out, lse, dqkv = run(qkv, dout, N, L, H, c.causal)
    qkv_v, qkv_f = _padded(qkv, 8)
    dout_v, dout_f = _padded(dout, 8)
    out_v, out_f = _padded(torch.zeros_like(out), 4)
    dqkv_v, dqkv_f = _padded(torch.zeros_like(dqkv), 4)
    lse_f = torch.full((N * H, L + 3), SENTINEL, device=dev)
    ws = torch.full((N * H, L + 3), SENTINEL, device=dev)
    ops.attention_fwd(qkv_v, N, L, H, c.causal, out=out_v, lse=lse_f, ld_lse=L + 3)
    ops.attention_bwd(qkv_v, out_v, dout_v, lse_f, N, L, H, c.causal, dqkv=dqkv_v, ws=ws, ld_lse=L + 3)
    assert torch.equal(out_v, out) and torch.equal(lse_f[:, :L], lse.view(N * H, L))
    assert torch.equal(dqkv_v.contiguous().view(torch.int16), dqkv.view(torch.int16))
    assert _pads_intact(out_f, D) and _pads_intact(dqkv_f, 3 * D) and _pads_intact(lse_f, L) and _pads_intact(ws, L)
    assert _pads_intact(qkv_f, 3 * D) and _pads_intact(dout_f, D)


@pytest.mark.parametrize("q_rows", [1, 17])
@pytest.mark.parametrize("c", CASE6[:2], ids=_id)
def test_rows_entries_through_strided_views(dev, c, q_rows):
    """mf_attention_fwd_rows (and, non-causal, mf_attention_bwd_rows) through the same strided views: the computed
    query tiles bit-identical to the full forward, everything else left as it was; dqkv bit-identical to the full
    backward on a dout with zeros at query rows >= q_rows, while those rows of dout, out and lse hold NaN."""
    N, L, H, D = c.N, c.L, c.H, 64 * c.H
    qkv, dout, _ = _case(c)
    out, lse = ops.attention_fwd(qkv, N, L, H, c.causal)
    qkv_v, _ = _padded(qkv, 8)
    out_v, out_f = _padded(torch.full_like(out, SENTINEL), 4)
    lse_f = torch.full((N * H, L + 3), SENTINEL, device=dev)
    ops.attention_fwd_rows(qkv_v, N, L, H, c.causal, q_rows, out_v, lse_f, ld_lse=L + 3)
    rows = min(L, (q_rows + 15) // 16 * 16)
    assert torch.equal(out_v.reshape(N, L, D)[:, :rows], out.view(N, L, D)[:, :rows])
    assert (out_f.view(N, L, D + 4)[:, rows:] == SENTINEL).all() and _pads_intact(out_f, D)
    assert torch.equal(lse_f[:, :rows], lse.view(N * H, L)[:, :rows]) and (lse_f[:, rows:] == SENTINEL).all()
    if c.causal:
        return
    d_ref = dout.clone().view(N, L, D)
    d_ref[:, q_rows:] = 0
    expect = ops.attention_bwd(qkv, out, d_ref.view(N * L, D), lse, N, L, H, False)
    nan = float("nan")
    dout_v, _ = _padded(dout, 8)
    out_v, _ = _padded(out, 4)
    lse_f[:, :L] = lse.view(N * H, L)
    dout_v.view(N, L, D)[:, q_rows:] = nan
    out_v.view(N, L, D)[:, q_rows:] = nan
    lse_f[:, q_rows:L] = nan
    dqkv_v, dqkv_f = _padded(torch.zeros_like(qkv), 4)
    ops.attention_bwd_rows(qkv_v, out_v, dout_v, lse_f, N, L, H, False, q_rows, dqkv=dqkv_v, ld_lse=L + 3)
    assert torch.equal(dqkv_v.contiguous().view(torch.int16), expect.view(torch.int16))
    assert _pads_intact(dqkv_f, 3 * D) and (lse_f[:, L:] == SENTINEL).all()


# ------------------------------------------------------------------ 7: fused in-projection + attention, range edges
@pytest.mark.parametrize("N,L,H,causal", CASE7)
def test_fused_in_projection_at_range_edges(dev, N, L, H, causal):
    """mf_qkv_attention_fwd at the ends of its two ranges (193 and 208 vision rows, 65 and 80 causal text rows), x of
    exactly N L rows so the last sequence's padded rows lie past the buffer (they read as zeros): qkv, out and lse
    bit-identical to mf_gemm_nt + mf_attention_fwd, and out and lse against fp64 from the kernel's own stored qkv."""
    D = 64 * H
    x, w, b = (t.to(dev) for t in host_inputs_fused(N, L, H))
    qkv_ref = ops.gemm_nt(x, w, bias=b, epilogue=ops.EPI_BIAS)
    o_ref, lse_ref = ops.attention_fwd(qkv_ref, N, L, H, causal)
    assert ops.qkv_attention_supported(N, L, H, causal)
    nan = float("nan")
    qkv = torch.full_like(qkv_ref, nan)
    out = torch.full((N * L, D), nan, device=dev, dtype=torch.float16)
    lse = torch.full((N * H * L,), nan, device=dev, dtype=torch.float32)
    ops.qkv_attention_fwd(x, w, b, qkv, out, lse, N, L, H, causal)
    assert torch.equal(qkv, qkv_ref) and torch.equal(out, o_ref) and torch.equal(lse, lse_ref)
    bound = {k: BOUND_UNIT[k] for k in ("lse", "out")}
    check(as_heads(out, lse, None, N, L, H), ref64(qkv, None, N, L, H, causal), bound, f"fused N{N} L{L} H{H}")
