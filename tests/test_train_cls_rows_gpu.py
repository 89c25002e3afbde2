"""The training step's last vision block on the class-token rows (engine.py _Tower.train_cls_rows) and the kernel it
adds, mf_attention_bwd_rows.  Both are exactness claims, so every comparison is bit for bit:

  * mf_attention_bwd_rows against mf_attention_bwd on a dout zeroed beyond q_rows, with the rows it promises not to
    read (dout, out, lse at queries >= q_rows) poisoned with NaN / Inf;
  * a train step with the attribute on against one with it off: loss, every gradient, the updated weights and the
    momentum, eager and as a captured graph, and the full forward() afterwards (stale rows of the class-row step do
    no harm).
"""
import pytest
import torch

from federated_multi_modal_amd import ops
from federated_multi_modal_amd import synthetic as syn
from federated_multi_modal_amd._lib import MapfedError
from federated_multi_modal_amd.engine import EngineConfig, MapleEngine

pytestmark = pytest.mark.gpu

N_ATT, H_ATT = 2, 12


@pytest.fixture(scope="module")
def attn_case(dev):
    """qkv / out / lse / dout of N = 2, H = 12 per sequence length, computed once and left unchanged."""
    cache = {}

    def get(L):
        if L not in cache:
            g = torch.Generator(device="cpu").manual_seed(1000 + L)
            D = H_ATT * 64
            qkv = torch.randn(N_ATT * L, 3 * D, generator=g).half().to(dev)
            dout = torch.randn(N_ATT * L, D, generator=g).half().to(dev)
            out, lse = ops.attention_fwd(qkv, N_ATT, L, H_ATT, False)
            cache[L] = (qkv, out, lse, dout)
        return cache[L]
    return get


@pytest.mark.parametrize("L", [199, 50, 17])
@pytest.mark.parametrize("q_rows", [1, 16, 17, "L"])
def test_attention_bwd_rows_bit_identical(dev, attn_case, L, q_rows):
    """dqkv as int16 bit patterns (a signed zero counts): the reference is the full backward on a dout with exact
    zeros at query rows >= q_rows; the row variant gets NaN in dout and out and +inf / NaN in lse at those rows."""
    q_rows = L if q_rows == "L" else q_rows
    N, H, D = N_ATT, H_ATT, H_ATT * 64
    qkv, out, lse, dout = attn_case(L)
    d_ref = dout.clone().view(N, L, D)
    d_ref[:, q_rows:] = 0
    ref = ops.attention_bwd(qkv, out, d_ref.view(N * L, D), lse, N, L, H, False)

    d_bad, o_bad, l_bad = dout.clone().view(N, L, D), out.clone().view(N, L, D), lse.clone().view(N * H, L)
    d_bad[:, q_rows:] = float("nan")
    o_bad[:, q_rows:] = float("nan")
    l_bad[:, q_rows:] = float("inf")
    l_bad[:, q_rows + 1::2] = float("nan")
    got = torch.full_like(ref, float("nan"))
    ops.attention_bwd_rows(qkv, o_bad.view(N * L, D), d_bad.view(N * L, D), l_bad.view(-1), N, L, H, False, q_rows,
                           dqkv=got)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    if q_rows < L:  # +0 in dQ at the dead query rows
        assert (got.view(N, L, 3 * D)[:, q_rows:, :D].reshape(-1).view(torch.int16) == 0).all()


def test_attention_bwd_rows_rejects_causal_and_long(dev, attn_case):
    """A causal mask and sequences past the fused kernel's 224 rows are errors (include/mapfed.h), not a detour
    through the full backward, which would read the dead rows."""
    qkv, out, lse, dout = attn_case(50)
    with pytest.raises(MapfedError):
        ops.attention_bwd_rows(qkv, out, dout, lse, N_ATT, 50, H_ATT, True, 1)
    L = 225
    D = H_ATT * 64
    z = torch.zeros(L, 3 * D, device=dev, dtype=torch.float16)
    with pytest.raises(MapfedError):
        ops.attention_bwd_rows(z, z[:, :D], z[:, :D], torch.zeros(H_ATT * L, device=dev), 1, L, H_ATT, False, 1)
    with pytest.raises(MapfedError):
        ops.attention_bwd_rows(qkv, out, dout, lse, N_ATT, 50, H_ATT, False, 51)


STATE = ("loss_out", "gflat16", "gflat32", "flat16", "flat32", "mom16", "mom32")


def _snap(e):
    torch.cuda.synchronize()
    return {k: getattr(e, k).clone() for k in STATE}


@pytest.fixture(scope="module", params=[3, 9], ids=["J3", "J9"])
def pair(request, dev):
    """Two identically built engines at (J, K, B) = (J, 10, 4), the second with train_cls_rows off, driven through
    the same two batches: two eager train steps, then two replays of each engine's captured step, then forward()."""
    J, K, B, seed = request.param, 10, 4, 5
    names = syn.synthetic_classnames(K, seed)
    batches = [syn.client_batch(seed, 0, r, B, K) for r in range(2)]
    res = []
    for on in (True, False):
        e = MapleEngine(EngineConfig(batch=B, classnames=names, prompt_depth=J, seed=seed), device=dev)
        assert e.vis.train_cls_rows and not e.txt.train_cls_rows
        e.vis.train_cls_rows = on
        e.set_lr(0.0026)
        r = {"eager": [], "graph": []}
        for b in batches:
            e.load_batch(torch.from_numpy(b.images), torch.from_numpy(b.labels))
            e.train_step()
            r["eager"].append(_snap(e))
        r["cls_fwd"] = e.vis._cls_fwd
        g = e.capture_train_step()
        for b in batches:
            e.load_batch(torch.from_numpy(b.images), torch.from_numpy(b.labels))
            g.replay()
            r["graph"].append(_snap(e))
        r["logits"] = e.forward().clone()
        r["full_fwd"] = not e.vis._cls_fwd
        torch.cuda.synchronize()
        res.append(r)
        del g, e
    return res


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_train_step_bit_identical_to_full_block(pair, mode):
    on, off = pair
    assert on["cls_fwd"] and not off["cls_fwd"]  # the two engines did take the two paths
    for step, (a, b) in enumerate(zip(on[mode], off[mode])):
        for k in STATE:
            view = torch.int16 if a[k].dtype == torch.float16 else torch.int32
            assert torch.equal(a[k].view(view), b[k].view(view)), (mode, step, k)
        assert torch.isfinite(a["loss_out"][0]) and a["loss_out"][3] == 0


def test_forward_after_class_row_step_is_the_full_forward(pair):
    """forward() after class-row training steps runs the full last block (existing tests read every block's
    output) and gives the logits of the engine that never took the class-row path."""
    on, off = pair
    assert on["full_fwd"] and off["full_fwd"]
    assert torch.equal(on["logits"], off["logits"])
