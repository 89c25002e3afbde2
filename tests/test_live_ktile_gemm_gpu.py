"""The dead-row forms of the class-row block's weight and bias gradients.  All three are exactness claims, so every
comparison is torch.equal on the raw bits of the fp16 / fp32 outputs against the existing full entry, run on the same
operands:

  * mf_gemm_splitk_live (K-tiles without a live k-row are skipped) against mf_gemm_splitk;
  * mf_colsum_f16_live (64-row chunks without a live row store +0 and read nothing) against mf_colsum_f16;
  * a bias gradient whose reduction is deferred to mf_col_reduce_batch (ColReduceDesc's fp16 flag, LNGradBatch.colsum)
    against mf_colsum_f16's own colsum_part_kernel + col_reduce_kernel<true>.
"""
import pytest
import torch

from federated_multi_modal_amd import ops
from federated_multi_modal_amd._lib import MapfedError, call

pytestmark = pytest.mark.gpu

# (L_full, L_live, seqs): K (or the row count) = seqs * L_full
LIVE_CASES = [
    (199, 1, 8),    # K = 1 592, ragged last tile
    (199, 16, 4),   # wider live prefix
    (130, 3, 5),    # live runs at tile offsets 0, 2, 4, 6, 8
    (126, 3, 5),    # a live run that straddles a tile edge (sequence 1: k = 126, 127 | 128)
    (64, 1, 6),     # tile-aligned rows
    (50, 1, 8),     # every tile live: the degenerate case
    (17, 1, 12),    # short sequences
    (400, 1, 3),    # splits = 8 at K = 1 200: ksplit = 192, slice 1 (rows 192..383) has no live tile
]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _dead_row_operand(dev, L_full, L_live, seqs, cols, m_live, seed):
    """[seqs * L_full, cols] fp16: seeded random live rows (row % L_full < L_live), zeros elsewhere with -0.0 in about
    a third of the dead entries; the columns >= m_live are dense."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    K = seqs * L_full
    a = torch.randn(K, cols, generator=g).half()
    dead = (torch.arange(K) % L_full >= L_live)[:, None].expand(K, cols).clone()
    dead[:, m_live:] = False
    zeros = torch.where(torch.rand(K, cols, generator=g) < 0.33, -0.0, 0.0).half()
    a = torch.where(dead, zeros, a)
    assert bool((a[dead].view(torch.int16) == -32768).any()) or not bool(dead.any())
    return a.to(dev)


@pytest.fixture(scope="module")
def operands(dev):
    """Per (case, M, m_live): A [K, M] with dead rows, B [K, 256] dense; built once and left unchanged."""
    cache = {}

    def get(case, M, m_live):
        key = (case, M, m_live)
        if key not in cache:
            L_full, L_live, seqs = case
            A = _dead_row_operand(dev, L_full, L_live, seqs, M, m_live, 7000 + 13 * L_full + M + m_live)
            g = torch.Generator(device="cpu").manual_seed(9000 + L_full)
            B = torch.randn(seqs * L_full, 256, generator=g).half().to(dev)
            cache[key] = (A, B)
        return cache[key]
    return get


@pytest.mark.parametrize("case", LIVE_CASES, ids=lambda c: "L%d_live%d_n%d" % c)
def test_gemm_splitk_live_bit_identical(dev, operands, case):
    L_full, L_live, seqs = case
    K = seqs * L_full
    for M, N, m_live in [(128, 128, 128), (128, 256, 128), (256, 128, 256), (256, 256, 256), (256, 256, 128),
                         (256, 128, 128)]:
        A, Bfull = operands(case, M, m_live)
        B = Bfull[:, :N]
        for splits in (0, 3, 4, 8):
            n_ws = ops.gemm_splitk_ws_floats(M, N, K, splits)
            for dt in (torch.float16, torch.float32):
                ws_ref = torch.full((n_ws,), float("nan"), device=dev)
                ws_got = torch.full((n_ws,), float("nan"), device=dev)  # an empty slice must store its +0 plane
                ref = torch.full((M, N), float("nan"), device=dev, dtype=dt)
                got = torch.full((M, N), float("nan"), device=dev, dtype=dt)
                ops.gemm_splitk(A, B, ref, ws_ref, splits=splits, a_kmajor=True, b_kmajor=True)
                ops.gemm_splitk(A, B, got, ws_got, splits=splits, a_kmajor=True, b_kmajor=True,
                                live=(L_live, L_full), m_live=m_live)
                tag = (case, M, N, m_live, splits, dt)
                assert torch.equal(_bits(ws_got), _bits(ws_ref)), tag
                assert torch.equal(_bits(got), _bits(ref)), tag
                assert bool(torch.isfinite(ref).all()), tag


def test_gemm_splitk_live_rejects(dev):
    L_full, L_live, seqs, M, N = 64, 1, 4, 128, 128
    K = seqs * L_full
    A = torch.zeros(K, M, device=dev, dtype=torch.float16)
    B = torch.zeros(K, N, device=dev, dtype=torch.float16)
    At, Bt = A.t().contiguous(), B.t().contiguous()
    C = torch.empty(M, N, device=dev, dtype=torch.float16)
    ws = torch.empty(ops.gemm_splitk_ws_floats(M, N, K), device=dev)
    ops.gemm_splitk(A, B, C, ws, a_kmajor=True, b_kmajor=True, live=(L_live, L_full))  # the accepted form
    with pytest.raises(MapfedError):  # a row-major A
        ops.gemm_splitk(At, B, C, ws, a_kmajor=False, b_kmajor=True, live=(L_live, L_full))
    with pytest.raises(MapfedError):  # a row-major B
        ops.gemm_splitk(A, Bt, C, ws, a_kmajor=True, b_kmajor=False, live=(L_live, L_full))
    with pytest.raises(MapfedError):  # K % L_full != 0
        ops.gemm_splitk(A, B, C, ws, a_kmajor=True, b_kmajor=True, live=(1, 60))
    with pytest.raises(MapfedError):  # L_live > L_full
        ops.gemm_splitk(A, B, C, ws, a_kmajor=True, b_kmajor=True, live=(65, 64))
    with pytest.raises(MapfedError):  # L_live = 0
        ops.gemm_splitk(A, B, C, ws, a_kmajor=True, b_kmajor=True, live=(0, 64))


@pytest.mark.parametrize("case", LIVE_CASES, ids=lambda c: "L%d_live%d_n%d" % c)
def test_colsum_live_bit_identical(dev, case):
    L_full, L_live, seqs = case
    R = seqs * L_full
    for C in (256, 1024):
        wide = _dead_row_operand(dev, L_full, L_live, seqs, C + 8, C + 8, 500 + L_full + C)
        for x in (wide[:, :C].contiguous(), wide[:, :C]):  # ld = C and ld > C
            for dt in (torch.float16, torch.float32):
                n_ws = ops.colsum_ws_floats(R, C)
                ws_ref = torch.full((n_ws,), float("nan"), device=dev)
                ws_got = torch.full((n_ws,), float("nan"), device=dev)
                ref = torch.full((C,), float("nan"), device=dev, dtype=dt)
                got = torch.full((C,), float("nan"), device=dev, dtype=dt)
                ops.colsum(x, ref, ws_ref)
                ops.colsum(x, got, ws_got, live=(L_live, L_full))
                assert torch.equal(_bits(ws_got), _bits(ws_ref)), (case, C, dt)
                assert torch.equal(_bits(got), _bits(ref)), (case, C, dt)
    with pytest.raises(MapfedError):  # R % L_full != 0
        ops.colsum(x[:R - 1], got, ws_got, live=(L_live, L_full))
    with pytest.raises(MapfedError):  # L_live > L_full
        ops.colsum(x, got, ws_got, live=(L_full + 1, L_full))


@pytest.mark.parametrize("rows", [64, 1000, 6368])
def test_deferred_bias_gradient_bit_identical(dev, rows):
    """colsum_part_kernel + col_reduce_kernel<true> (mf_colsum_f16) against the partials + one mf_col_reduce_batch
    launch with the fp16 flag.  6 368 rows are 100 chunks: the unrolled four-accumulator loop and its tail both run.
    A second, wider fp32 entry shares the launch (another C, the flag clear)."""
    C = 768
    g = torch.Generator(device="cpu").manual_seed(40 + rows)
    x = torch.randn(rows, C, generator=g).half().to(dev)
    x2 = torch.randn(rows, 2 * C, generator=g).half().to(dev)
    ref = torch.full((C,), float("nan"), device=dev, dtype=torch.float16)
    ref2 = torch.full((2 * C,), float("nan"), device=dev, dtype=torch.float32)
    ops.colsum(x, ref)
    ops.colsum(x2, ref2)
    got = torch.full((C,), float("nan"), device=dev, dtype=torch.float16)
    got2 = torch.full((2 * C,), float("nan"), device=dev, dtype=torch.float32)
    lnb = ops.LNGradBatch(dev)
    lnb.colsum(x, got)
    lnb.colsum(x2, got2)
    assert call("mf_colsum_blocks", rows) == (rows + 63) // 64 and len(lnb.descs) == 2
    assert bool(torch.isnan(got).all())  # nothing is reduced before finish()
    lnb.finish()
    assert torch.equal(_bits(got), _bits(ref))
    assert torch.equal(_bits(got2), _bits(ref2))
    # a second pass through the same table (the captured step replays it) with other data
    x.mul_(-0.5)
    ops.colsum(x, ref)
    lnb.colsum(x, got)
    lnb.colsum(x2, got2)
    lnb.finish()
    assert torch.equal(_bits(got), _bits(ref))
    assert torch.equal(_bits(got2), _bits(ref2))
