"""CPU pins of what tests/test_gpu_helpers.py relies on (tests/helpers_cases.py): the float64 references agree with independent
implementations, every bound is finite and non-negative, and no case can pass because its bound is loose."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import helpers_cases as HC
from tests import util as U

# stands in for the measured exponential error in the cap check: far above anything a working exponential shows (tests/test_gpu_helpers.py
# EXPF_ULPS_GRANTED), so the cap is checked against a larger limit than the GPU test grants
EXPF_ULPS_FOR_CAP = 256.0


def test_tps_grid_reference_matches_the_oracle_grid_generator():
    """float64 formula of the kernel's comment vs oracle/warp.py's TPSGridGen restatement (fp32, range 0.9 lattice) at N = 25, 16 x 12"""
    from oracle import warp
    H, W = 16, 12
    ctrl_o, inv_o, rep = warp.tps_grid_matrices(H, W)
    ctrl = HC.tps_lattice(5, 0.9)
    assert torch.allclose(ctrl.float(), ctrl_o, atol=1e-6)
    inv = HC.tps_inverse_kernel(ctrl)
    assert float((inv.float() - inv_o).abs().max()) <= 1e-3 * float(inv_o.abs().max())
    coor = (ctrl[None] + HC.randn((2, 25, 2), 7, 0.1).double()).float()
    ref, bound = HC.tps_grid_ref_bound(coor, inv.float(), ctrl.float(), H, W)
    y = torch.cat([coor, torch.zeros(2, 3, 2)], 1)
    want = torch.matmul(rep, torch.matmul(inv_o, y)).view(2, H, W, 2)
    assert float((ref - want.double()).abs().max()) <= 2e-4
    assert float(ref.abs().max()) > 0.5


def test_tps_phi_is_zero_where_a_pixel_is_a_control_point():
    coor, inv, ctrl, ref, bound = HC.tps_case(25, 5, 5)
    xs = torch.arange(5, dtype=torch.float32) * 2 / 4 - 1                       # the kernel's fp32 pixel coordinates
    assert sorted(set(ctrl[:, 0].tolist())) == xs.tolist()                      # coincide with the lattice bit for bit
    # an identity warp (coor == ctrl) reproduces the pixel coordinates
    r, _ = HC.tps_grid_ref_bound(ctrl[None], inv, ctrl, 5, 5)
    Y, X = torch.meshgrid(xs.double(), xs.double(), indexing="ij")
    assert float((r[0] - torch.stack([X, Y], -1)).abs().max()) < 1e-5


def test_text_meta_reference_matches_argmax():
    ids = HC.text_meta_ids()
    first, eot = HC.text_meta_ref(ids, HC.TEXT_VSTAR, 1)
    assert first.tolist() == [70, 3, -1, -1, -1, -1]
    T = ids.shape[1]
    assert (eot.long() - torch.arange(6) * T).tolist() == [70, 3, int(ids[2].argmax()), 10, 65, 40]
    for b in range(6):                                                          # torch.argmax returns the first maximum as well
        assert int(eot[b]) - b * T == int((ids[b] == ids[b].max()).nonzero()[0])
    assert HC.text_meta_ref(ids, HC.TEXT_VSTAR, 0)[0].tolist() == [-1] * 6


@pytest.mark.parametrize("case", HC.SQ_CASES)
def test_single_query_reference_matches_sdpa(case):
    d, heads, Nk, n, _ = case
    q, kv, scale, ref, bound = HC.single_query_case(*case)
    H = heads * d
    qh = q.double().reshape(n, heads, 1, d)
    kh = kv[..., :H].double().reshape(n, Nk, heads, d).permute(0, 2, 1, 3)
    vh = kv[..., H:].double().reshape(n, Nk, heads, d).permute(0, 2, 1, 3)
    want = F.scaled_dot_product_attention(qh, kh, vh, scale=scale).reshape(n, H)
    assert float((ref - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_logit_case_reaches_forty():
    q, kv, scale, _, _ = HC.single_query_case(*HC.SQ_CASES[-1])
    d, heads, Nk, n, _ = HC.SQ_CASES[-1]
    s = torch.einsum("nhd,nkhd->nhk", q.reshape(n, heads, d), kv[..., :heads * d].reshape(n, Nk, heads, d)) * scale
    assert 30.0 <= float(s.max()) <= 60.0, float(s.max())


def test_image_post_reference_rounds_half_to_even():
    x = torch.tensor([[-1.0, 1.0, 0.0], [1.0 / 255 - 1.0, 3.0 / 255 - 1.0, 5.0]], dtype=torch.float16)
    f, u = HC.image_post_ref(x)
    assert f[0].tolist() == [0.0, 1.0, 0.5] and u[0].tolist() == [0, 255, 128]  # 127.5 -> 128 (even)
    assert int(u[1, 2]) == 255
    assert HC.all_finite_halves().shape == (21163, 3) and bool(torch.isfinite(HC.all_finite_halves().float()).all())


def test_patchify_and_text_embed_references():
    px = HC.randn((2, 3, 28, 28), 3)
    out = HC.patchify_ref(px, 14, 640)
    assert out.shape == (2, 5, 640) and not bool(out[:, 0].any()) and not bool(out[:, :, 588:].any())
    assert float(out[1, 4, 2 * 196 + 3 * 14 + 5]) == float(px[1, 2, 14 + 3, 14 + 5].half())
    ids = torch.tensor([[-5, 400, 7]], dtype=torch.int32)
    tok, pos, wemb = HC.randn((320, 8), 4, half=True).half(), HC.randn((3, 8), 5, half=True).half(), HC.randn((1, 4, 8), 6, half=True).half()
    e = HC.text_embed_ref(ids, torch.tensor([2]), 4, tok, pos, wemb)
    assert torch.equal(e[0, 0], (tok[0].float() + pos[0].float()).half()) and torch.equal(e[0, 1], (tok[319].float() + pos[1].float()).half())
    assert torch.equal(e[0, 2], (wemb[0, 0].float() + pos[2].float()).half())   # the window runs past the sentence: rows 1-3 are unused


def test_every_bound_is_finite_nonnegative_and_tight():
    """limit = derived bound + the final rounding check_elem grants; it must stay below 2e-2 of the case's largest reference magnitude"""
    names = []
    for name, ref, bound, out_f32 in HC.bounded_cases(EXPF_ULPS_FOR_CAP):
        names.append(name)
        ref, bound = ref.double(), torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), name
        last = U.U32 * ref.abs() if out_f32 else U.ulp16(ref)
        peak = float(ref.abs().max())
        assert peak > 0, name
        assert float((bound + last).max()) < 2e-2 * peak, (name, float((bound + last).max()), peak)
    assert len(names) == len(set(names)) and len(names) >= 40


def test_small_linear_cases_cover_the_product_call_shapes():
    have = {c[:5] for c in HC.SL_CASES}
    for shape in [(1, 1, "silu", 0, 0), (1, 1, "none", 0, 0), (1, 1, "none", 1, 0), (0, 0, "none", 0, 0), (0, 0, "none", 0, 1),
                  (0, 0, "gelu", 0, 0), (0, 1, "tanh", 0, 0)]:
        assert shape in have, shape
    assert {c[2] for c in HC.SL_CASES} == {"none", "silu", "gelu", "relu", "tanh"}
    assert {c[5] for c in HC.SL_CASES} == {1, 8, 9, 19} and {c[6] for c in HC.SL_CASES} == {50, 4, 101} and {c[7] for c in HC.SL_CASES} == {8, 512, 520, 1280}
    assert {(c[0], c[1]) for c in HC.SL_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_guarded_accepts_an_unaligned_stride_only_on_request():
    g = U.guarded_out(5, 3, ld=3, dtype=torch.float32, device="cpu", any_ld=True)
    assert g.ptr % 16 == 0 and g.ld == 3
    U.assert_untouched(g)
    with pytest.raises(AssertionError):
        U.guarded_out(5, 3, ld=3, dtype=torch.float32, device="cpu")
