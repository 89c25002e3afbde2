"""The small-M projection kernel (csrc/gemm.hip gemm_sm_kernel, what mf_gemm's heuristic picks for row-major products
of at most 64 rows) against the 64x64 tile kernel (explicit tile 3): every output bit for bit, for every epilogue, on
contiguous rows and on rows strided by 199 * 768 elements (the class-row views of the vision tower's buffers)."""
import pytest
import torch

from federated_multi_modal_amd import ops

pytestmark = pytest.mark.gpu

LD = 199 * 768
MMAX = 64
EPIS = (ops.EPI_NONE, ops.EPI_BIAS, ops.EPI_BIAS_RESID, ops.EPI_BIAS_GELU, ops.EPI_DGELU, ops.EPI_F32, ops.EPI_RESID)


@pytest.fixture(scope="module")
def pool(dev):
    """Operands for every case, made once and only read: A / residual rows and weights for the largest shape, as
    flat buffers the cases take contiguous or strided views of."""
    g = torch.Generator(device="cpu").manual_seed(11)
    flat = lambda: (torch.randn(MMAX * LD + 3072, generator=g) * 0.5).half().to(dev)
    return {"A": flat(), "R": flat(), "W": (torch.randn(3072 * 3072, generator=g) * 0.03).half().to(dev),
            "b": (torch.randn(3072, generator=g) * 0.02).half().to(dev)}


def _rows(buf, M, cols, strided):
    return torch.as_strided(buf, (M, cols), (LD if strided else cols, 1))


@pytest.mark.parametrize("N,K", [(768, 768), (3072, 768), (768, 3072), (512, 768)])
@pytest.mark.parametrize("M", [1, 17, 32, 33, 64])
def test_small_m_gemm_bit_identical_to_tile3(dev, pool, M, N, K):
    W = pool["W"][:N * K].view(N, K)
    b = pool["b"][:N]
    for strided in (False, True):
        A, R = _rows(pool["A"], M, K, strided), _rows(pool["R"], M, N, strided)
        for epi in EPIS:
            kw = {"bias": b} if epi in (ops.EPI_BIAS, ops.EPI_BIAS_RESID, ops.EPI_BIAS_GELU) else {}
            if epi in (ops.EPI_BIAS_RESID, ops.EPI_DGELU, ops.EPI_RESID):
                kw["aux_in"] = R
            res = []
            for tile in (0, 3):  # 0: the heuristic's pick, the small-M kernel at M <= 64
                dt = torch.float32 if epi == ops.EPI_F32 else torch.float16
                C = _rows(torch.full((MMAX * LD + 3072,), 7.0, device=dev, dtype=dt), M, N, strided)
                aux_out = None
                if epi == ops.EPI_BIAS_GELU:
                    aux_out = _rows(torch.full((MMAX * LD + 3072,), 7.0, device=dev, dtype=torch.float16), M, N,
                                    strided)
                ops.gemm_nt(A, W, C, aux_out=aux_out, epilogue=epi, tile=tile, **kw)
                res.append((C, aux_out))
            (c0, x0), (c3, x3) = res
            assert torch.isfinite(c3).all() and not (c3 == 7.0).all()
            assert torch.equal(c0, c3), (M, N, K, epi, strided)
            if x0 is not None:
                assert torch.equal(x0, x3), (M, N, K, epi, strided, "aux_out")
            if strided:  # nothing written between the rows
                gap = torch.as_strided(c0, (M, LD - N), (LD, 1), c0.storage_offset() + N)
                assert (gap == 7.0).all()


def test_small_m_gemm_explicit_tile_and_limits(dev, pool):
    """Tile 50 names the kernel (the A/B handle); more than 64 rows or K past 3072 is an error there, and the
    heuristic sends such products to the tile kernels."""
    from federated_multi_modal_amd._lib import MapfedError
    W = pool["W"][:768 * 768].view(768, 768)
    A = _rows(pool["A"], 32, 768, False)
    assert torch.equal(ops.gemm_nt(A, W, tile=50), ops.gemm_nt(A, W, tile=3))
    with pytest.raises(MapfedError):
        ops.gemm_nt(_rows(pool["A"], 65, 768, False), W, tile=50)
    W4 = pool["W"][:64 * 4096].view(64, 4096)
    A4 = _rows(pool["A"], 8, 4096, False)
    with pytest.raises(MapfedError):
        ops.gemm_nt(A4, W4, tile=50)
    assert torch.equal(ops.gemm_nt(A4, W4), ops.gemm_nt(A4, W4, tile=3))
