"""Few-step sampling on the host (no GPU): LCM and TCD (scheduler kinds 7 and 8), trailing timestep spacing (bit 6) and one-step runs through
the C ABI (ladi_sched_timesteps, ladi_sched_table_from, ladi_sched_keep_coeffs) and the mirrors (ladi_vton_amd/schedulers.py) against the
float64 restatement in tests/few_step_ref.py, plus known answers that do not depend on that restatement."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import pipeline as P
from tests import few_step_ref as R

DDIM, PNDM, LMS, DPM, EULER, EULER_A, LCM, TCD = 0, 1, 2, 3, 4, 5, 7, 8
TRAILING = 1 << 6
ORIG = lambda o: (o << 12)          # noqa: E731  (bits 12-21: original_inference_steps)
F32 = lambda v: float(np.float32(v))          # noqa: E731  (eta as the C ABI carries it)


def lib_error():
    from ladi_vton_amd import _lib
    return _lib.last_error()


def _timesteps(lib, code, n):
    buf = (ctypes.c_int * (n + 2))()
    cnt = lib.ladi_sched_timesteps(code, n, buf, n + 2)
    return cnt, list(buf[:max(cnt, 0)])


def _table_from(lib, code, n, eta=0.0, first_step=0):
    ac = P.alphas_cumprod().contiguous()
    ts, rows, start = (ctypes.c_double * (n + 2))(), (ctypes.c_float * (10 * (n + 2)))(), (ctypes.c_float * 3)()
    cnt = lib.ladi_sched_table_from(code, n, ctypes.c_void_p(ac.data_ptr()), eta, first_step, ts, rows, n + 2, start)
    if cnt < 0:
        return cnt, lib_error()
    return list(ts[:cnt]), np.array(list(rows[:10 * cnt]), dtype=np.float64).reshape(cnt, 10), [float(v) for v in start]


def _close(got, want, what):
    """relative error <= 1e-6 (tests/test_cpu_preserve.py's bound for fp32-held double coefficients); an exact zero stays one"""
    if want == 0.0:
        assert got == 0.0, (what, got)
    else:
        assert abs(got - want) <= 1e-6 * abs(want), (what, got, want)


# ------------------------------------------------------------------------------------------------------------------ timesteps
@pytest.mark.parametrize("orig,n,want", [(50, 1, [999]), (50, 2, [999, 499]), (50, 3, [999, 679, 339]), (50, 4, [999, 759, 499, 259]),
                                         (50, 8, [999, 879, 759, 639, 499, 379, 259, 139]), (100, 4, [999, 749, 499, 249])])
def test_lcm_tcd_timesteps_exact(lib, orig, n, want):
    import ladi_vton_amd as L
    for kind, cls in ((LCM, L.LCMScheduler), (TCD, L.TCDScheduler)):
        assert _timesteps(lib, kind | ORIG(orig), n) == (n, want)
        if orig == 50:
            assert _timesteps(lib, kind, n) == (n, want)                 # 0 means 50
        s = cls(original_inference_steps=orig)
        s.set_timesteps(n)
        assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want
        assert s.config.original_inference_steps == orig and s.kind & 15 == kind
    assert R.lcm_timesteps(n, orig) == want


@pytest.mark.parametrize("orig", [7, 40, 50, 100, 1000])
def test_lcm_timesteps_equal_the_numpy_form_for_every_n(lib, orig):
    for n in range(1, orig + 1):
        assert _timesteps(lib, LCM | ORIG(orig), n)[1] == R.lcm_timesteps(n, orig), n


@pytest.mark.parametrize("n,want", [(1, [999]), (3, [999, 666, 332]), (4, [999, 749, 499, 249]), (8, [999, 874, 749, 624, 499, 374, 249, 124])])
def test_trailing_timesteps_exact(lib, n, want):
    import ladi_vton_amd as L
    for kind in (DDIM, EULER, EULER_A):
        assert _timesteps(lib, kind | TRAILING, n) == (n, want)
    assert R.trailing_timesteps(n) == want
    assert [int(v) for v in np.round(np.arange(1000, 0, -1000 / n)) - 1] == want        # diffusers' form, equal for every n <= 47
    s = L.DDIMScheduler(timestep_spacing="trailing")
    s.set_timesteps(n)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want and s.config.timestep_spacing == "trailing"
    for cls in (L.EulerDiscreteScheduler, L.EulerAncestralDiscreteScheduler):
        e = cls(timestep_spacing="trailing")
        e.set_timesteps(n)
        assert e.timesteps.tolist() == [float(t) for t in want] and e.config.timestep_spacing == "trailing"
        assert abs(e.init_noise_sigma - 14.6146) < 1e-4 and float(e.sigmas[-1]) == 0.0 and len(e.sigmas) == n + 1


@pytest.mark.parametrize("n", [1, 2, 3, 7, 47, 48, 61, 1000])
def test_trailing_timesteps_no_duplicate_no_negative(lib, n):
    cnt, ts = _timesteps(lib, DDIM | TRAILING, n)
    assert cnt == n and ts == R.trailing_timesteps(n)
    assert ts[0] == 999 and min(ts) >= 0 and all(a > b for a, b in zip(ts, ts[1:]))


def test_step_count_ranges(lib):
    for kind in (LCM, TCD):
        assert _timesteps(lib, kind, 51)[0] < 0 and "num_inference_steps" in lib_error()
        assert _timesteps(lib, kind, 50)[0] == 50
        assert _timesteps(lib, kind | ORIG(7), 8)[0] < 0 and _timesteps(lib, kind | ORIG(7), 7)[0] == 7
        assert _timesteps(lib, kind, 0)[0] < 0
        assert _timesteps(lib, kind | ORIG(1000), 1000)[0] == 1000
        assert _timesteps(lib, kind | ORIG(1001), 4)[0] < 0 and "scheduler" in lib_error()
    assert _timesteps(lib, DDIM | TRAILING, 1000)[0] == 1000 and _timesteps(lib, DDIM | TRAILING, 1001)[0] < 0
    assert _timesteps(lib, DDIM | TRAILING, 0)[0] < 0
    for code in (DDIM, PNDM, DPM):                                # the plain codes keep [2, 1000] and today's message
        assert _timesteps(lib, code, 1)[0] < 0 and "num_inference_steps out of range [2, 1000]" in lib_error()
    for code in range(6):
        got = _table_from(lib, code, 1)
        assert got[0] < 0 and "num_inference_steps out of range [2, 1000]" in got[1], (code, got)
    import ladi_vton_amd as L
    with pytest.raises(L.NativeError, match="num_inference_steps"):
        L.LCMScheduler().set_timesteps(51)


@pytest.mark.parametrize("code", [DDIM | ORIG(50), DPM | ORIG(1), EULER | ORIG(100), PNDM | TRAILING, LMS | TRAILING, DPM | TRAILING, LCM | TRAILING,
                                  TCD | TRAILING, LCM | (1 << 4), TCD | (1 << 7), DDIM | TRAILING | (1 << 4), LCM | (1 << 8), TCD | (1 << 22),
                                  6, 9, 15])
def test_invalid_few_step_codes_rejected(lib, code):
    assert _timesteps(lib, code, 4)[0] < 0 and "scheduler" in lib_error(), (code, lib_error())
    got = _table_from(lib, code, 4)
    assert got[0] < 0 and "scheduler" in got[1], (code, got)
    out = (ctypes.c_float * 16)()
    assert lib.ladi_sched_keep_coeffs(code, 4, None, 0, out, 8) < 0


def test_eta_rule(lib):
    """a non-zero eta: DDIM (any >= 0) and TCD (its gamma, [0, 1]) only"""
    assert _table_from(lib, TCD, 4, eta=1.0)[0] != -1 and len(_table_from(lib, TCD, 4, eta=1.0)[0]) == 4
    got = _table_from(lib, TCD, 4, eta=1.5)
    assert got[0] < 0 and "[0, 1]" in got[1]
    assert _table_from(lib, TCD, 4, eta=-0.1)[0] < 0
    assert len(_table_from(lib, DDIM | TRAILING, 4, eta=1.5)[0]) == 4
    for code in (LCM, EULER | TRAILING, EULER_A | TRAILING):
        got = _table_from(lib, code, 4, eta=0.3)
        assert got[0] < 0 and "eta" in got[1], (code, got)


# ------------------------------------------------------------------------------------------------------------------ rows
def _ref_of(case, eta):
    if case == "lcm":
        return R.RefLCM()
    if case == "tcd":
        return R.RefTCD(gamma=F32(eta))
    if case == "ddim":
        return R.RefDDIM(eta=F32(eta), trailing=True)
    return R.RefEuler(ancestral=case == "euler_a")


CODE = {"lcm": LCM, "tcd": TCD, "ddim": DDIM | TRAILING, "euler": EULER | TRAILING, "euler_a": EULER_A | TRAILING}
ROW_CASES = ([("lcm", 0.0, n) for n in (1, 2, 4, 8)] + [("tcd", eta, n) for eta in (0.0, 0.3, 1.0) for n in (1, 2, 4, 8)]
             + [("ddim", eta, n) for eta in (0.0, 0.5) for n in (1, 3, 4)] + [(c, 0.0, n) for c in ("euler", "euler_a") for n in (1, 3, 4)])


@pytest.mark.parametrize("case,eta,n", ROW_CASES)
def test_native_rows_match_restatement(lib, case, eta, n):
    """x' = c_x x + c_e w_0 eps + c_n noise_i: every coefficient against the one recovered from the restatement's recurrence, whole runs and
    tails (first_step 0, 1, n - 1), relative error <= 1e-6"""
    firsts = sorted({0, 1, n - 1} & set(range(n))) if case in ("lcm", "tcd") else [0]
    for first_step in firsts:
        ts, tb, start = _table_from(lib, CODE[case], n, eta=eta, first_step=first_step)
        ref = _ref_of(case, eta)
        ref.set_timesteps(n, first_step=first_step)
        assert ts == [float(t) for t in ref.timesteps] and len(tb) == n - first_step
        for i in range(len(ts)):
            c_x, c_e, c_n = R.row_of(ref, i)
            _close(tb[i, 0], c_x, (first_step, i, "c_x"))
            _close(tb[i, 1] * tb[i, 2], c_e, (first_step, i, "c_e"))
            _close(tb[i, 8], c_n, (first_step, i, "c_n"))
            assert not tb[i, 3:8].any()
            if case in ("euler", "euler_a"):
                want = 1.0 / (float(ref.sigmas[i + 1]) ** 2 + 1) ** 0.5 if i + 1 < len(ts) else 1.0
                _close(tb[i, 9], want, (i, "in_scale_next"))
            else:
                assert tb[i, 9] == 1.0
        if case == "lcm":
            assert tb[-1, 8] == 0.0 and (tb[:-1, 8] > 0).all()
        if case == "tcd" and eta == 0.0:
            assert not tb[:, 8].any()
        if case == "tcd" and eta > 0.0:
            assert tb[-1, 8] == 0.0 and (tb[:-1, 8] > 0).all()
        if case == "euler_a":
            assert tb[-1, 8] == 0.0                               # sigma_up of the step into sigma 0 (a one-step run has no noise term)
        # the start of the run (start_out): noise * init_noise_sigma for a whole run, add_noise at the first timestep for a tail
        if case in ("euler", "euler_a"):
            _close(start[0], 0.0, "k_x")
            _close(start[1], ref.init_noise_sigma, "k_n")
            assert abs(start[1] - 14.6146) < 1e-4
            _close(start[2], 1.0 / (float(ref.sigmas[0]) ** 2 + 1) ** 0.5, "in_scale0")
        elif first_step == 0:
            assert start == [0.0, 1.0, 1.0]
        else:
            a = float(ref.ac[ref.timesteps[0]])
            _close(start[0], a ** 0.5, "k_x")
            _close(start[1], (1 - a) ** 0.5, "k_n")
            assert start[2] == 1.0


def test_trailing_ddim_prev_is_t_minus_ratio(lib):
    """n = 3: prev = 666, 333, -1 (diffusers' t - T // n), not the next timestep 666, 332"""
    ts, tb, _ = _table_from(lib, DDIM | TRAILING, 3)
    ac = R.alphas_cumprod64()
    for i, prev in enumerate([666, 333, 0]):                     # prev < 0 uses alphas_cumprod[0]
        _close(tb[i, 0], (ac[prev] / ac[int(ts[i])]) ** 0.5, i)
    assert abs(tb[1, 0] - (ac[332] / ac[666]) ** 0.5) > 1e-4 * tb[1, 0]


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_tcd_eta_zero_is_a_ddim_jump_between_its_own_timesteps(lib, n):
    """known answer: gamma = 0 makes every TCD update the deterministic DDIM jump t_i -> t_{i+1}, the last one to t = 0"""
    ts, tb, _ = _table_from(lib, TCD, n, eta=0.0)
    ac = R.alphas_cumprod64()
    for i in range(n):
        t, tp = int(ts[i]), int(ts[i + 1]) if i + 1 < n else 0
        _close(tb[i, 0], (ac[tp] / ac[t]) ** 0.5, (i, "c_x"))
        _close(tb[i, 1] * tb[i, 2], (1 - ac[tp]) ** 0.5 - ac[tp] ** 0.5 * (1 - ac[t]) ** 0.5 / ac[t] ** 0.5, (i, "c_e"))
        assert tb[i, 8] == 0.0


# ------------------------------------------------------------------------------------------------------------------ mirrors
def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("n", [1, 2, 4])
def test_lcm_returns_x0_on_an_analytic_eps(n):
    """eps_i = (x_i - sqrt(a_t) x0) / sqrt(1 - a_t) makes every data prediction x0: the LCM mirror ends at x0 whatever the step noise"""
    import ladi_vton_amd as L
    s = L.LCMScheduler()
    s.set_timesteps(n)
    ac = R.alphas_cumprod64()
    rng = np.random.default_rng(5)
    x0 = rng.standard_normal((2, 4, 5, 6))
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        x = torch.tensor(rng.standard_normal(x0.shape), dtype=torch.float32)
        for t in s.timesteps:
            a = ac[int(t)]
            eps = (x.double().numpy() - a ** 0.5 * x0) / (1 - a) ** 0.5
            x = s.step(torch.tensor(eps, dtype=torch.float32), t, x, generator=g).prev_sample
        assert _rel(x.numpy(), x0) <= 1e-5, (n, seed, _rel(x.numpy(), x0))


@pytest.mark.parametrize("eta", [0.0, 0.3])
def test_tcd_last_step_lands_at_timestep_zero(eta):
    import ladi_vton_amd as L
    s = L.TCDScheduler()
    s.set_timesteps(4)
    ac = R.alphas_cumprod64()
    rng = np.random.default_rng(6)
    x0, x = rng.standard_normal((2, 4, 3, 3)), rng.standard_normal((2, 4, 3, 3))
    t = int(s.timesteps[-1])
    eps = (x - ac[t] ** 0.5 * x0) / (1 - ac[t]) ** 0.5
    g = torch.Generator().manual_seed(1)
    before = g.get_state()
    got = s.step(torch.tensor(eps, dtype=torch.float32), t, torch.tensor(x, dtype=torch.float32), eta=eta, generator=g).prev_sample
    assert _rel(got.numpy(), ac[0] ** 0.5 * x0 + (1 - ac[0]) ** 0.5 * eps) <= 1e-5
    assert torch.equal(g.get_state(), before)                     # the last evaluation draws nothing


def _mirror_and_ref(case, eta):
    import ladi_vton_amd as L
    if case == "lcm":
        return L.LCMScheduler(), R.RefLCM()
    if case == "tcd":
        return L.TCDScheduler(), R.RefTCD(gamma=F32(eta))
    if case == "ddim":
        return L.DDIMScheduler(timestep_spacing="trailing"), R.RefDDIM(eta=F32(eta), trailing=True)
    cls = L.EulerAncestralDiscreteScheduler if case == "euler_a" else L.EulerDiscreteScheduler
    return cls(timestep_spacing="trailing"), R.RefEuler(ancestral=case == "euler_a")


def _draws(case, eta, i, n):
    """does the mirror's step() draw at evaluation i of n"""
    if case in ("euler", "euler_a"):
        return True                                              # one draw per step, also for Euler (unused), as diffusers
    if case == "lcm":
        return i + 1 < n
    return eta > 0.0 and (case == "ddim" or i + 1 < n)


@pytest.mark.parametrize("case,eta", [("lcm", 0.0), ("tcd", 0.0), ("tcd", 0.3), ("tcd", 1.0), ("ddim", 0.0), ("ddim", 0.5), ("euler", 0.0),
                                      ("euler_a", 0.0)])
@pytest.mark.parametrize("n,first_step", [(1, 0), (2, 0), (4, 0), (8, 0), (4, 3), (8, 1)])
def test_mirror_trajectory_matches_restatement(case, eta, n, first_step):
    """same seed, same draw order over a random eps sequence: rel-L2 < 1e-5 at every step (test_euler_mirror_trajectory_matches_restatement's
    bound), and the generator ends where the reference's draws end"""
    s, ref = _mirror_and_ref(case, eta)
    s.set_timesteps(n, first_step=first_step) if first_step else s.set_timesteps(n)
    ref.set_timesteps(n, first_step=first_step)
    assert [float(t) for t in s.timesteps.tolist()] == [float(t) for t in ref.timesteps]
    assert abs(s.init_noise_sigma - ref.init_noise_sigma) < 1e-6
    shape, evals = (2, 4, 6, 5), n - first_step
    rng = np.random.default_rng(100 + n)
    eps = [rng.standard_normal(shape) for _ in range(evals)]
    x = torch.tensor(rng.standard_normal(shape) * s.init_noise_sigma, dtype=torch.float32)
    xr = x.double().numpy()
    g, gr = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    kw = {"eta": eta} if case in ("tcd", "ddim") else {}
    for i, t in enumerate(s.timesteps):
        assert _rel(s.scale_model_input(x, t).numpy(), ref.scale_model_input(x.double().numpy(), float(t))) < 1e-6
        x = s.step(torch.tensor(eps[i], dtype=torch.float32), t, x, generator=g, **kw).prev_sample
        noise = torch.randn(shape, generator=gr, dtype=torch.float32).double().numpy() if _draws(case, eta, i, evals) else np.zeros(shape)
        xr = ref.step(eps[i], float(t), xr, noise=noise)
        assert _rel(x.numpy(), xr) < 1e-5, (i, _rel(x.numpy(), xr))
    assert torch.equal(g.get_state(), gr.get_state())


@pytest.mark.parametrize("case", ["lcm", "tcd", "ddim", "euler", "euler_a"])
@pytest.mark.parametrize("n,first_step", [(1, 0), (4, 0), (4, 1), (4, 3), (8, 0)])
def test_keep_coeffs_of_the_new_codes(lib, case, n, first_step):
    """add_noise at timesteps[i + 1] (sqrt(a), sqrt(1 - a); the sigma kinds 1, sigma), the last row (1, 0): native table, mirror and
    restatement agree to 1e-6"""
    ac = P.alphas_cumprod().contiguous()
    out = (ctypes.c_float * (2 * (n + 2)))()
    cnt = lib.ladi_sched_keep_coeffs(CODE[case], n, ctypes.c_void_p(ac.data_ptr()), first_step, out, n + 2)
    assert cnt == n - first_step, lib_error()
    got = np.array(list(out[:2 * cnt]), dtype=np.float64).reshape(cnt, 2)
    s, ref = _mirror_and_ref(case, 0.0)
    s.set_timesteps(n, first_step=first_step) if first_step else s.set_timesteps(n)
    ref.set_timesteps(n, first_step=first_step)
    want = R.keep_coeffs(ref)
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    for i in range(cnt):
        _close(got[i, 0], want[i][0], (i, "k_x"))
        _close(got[i, 1], want[i][1], (i, "k_n"))
        if i + 1 < cnt:
            t = s.timesteps[i + 1]
            _close(float(s.add_noise(one, zero, t)), want[i][0], (i, "mirror k_x"))
            _close(float(s.add_noise(zero, one, t)), want[i][1], (i, "mirror k_n"))
    assert tuple(got[-1]) == (1.0, 0.0)


# ------------------------------------------------------------------------------------------------------------------ pipeline
class _Dist:
    def __init__(self, m):
        self.m = m

    def sample(self, noise=None):
        return self.m

    def mode(self):
        return self.m


class _VAE:
    config = SimpleNamespace(block_out_channels=[8, 8, 8, 8], scaling_factor=0.18215)

    def encode(self, x):
        return SimpleNamespace(latent_dist=_Dist(torch.nn.functional.avg_pool2d(x.float(), 8)[:, :1].repeat(1, 4, 1, 1))), None


class _UNet:
    config = SimpleNamespace(sample_size=4)

    def __call__(self, x, t, encoder_hidden_states=None, **kw):
        return SimpleNamespace(sample=0.1 * x[:, :4])


def _cpu_pipe(scheduler):
    """the pipeline with stand-in modules on the CPU: the modular path's host arithmetic and RNG order, nothing native"""
    import ladi_vton_amd as L

    class Pipe(L.StableDiffusionTryOnePipeline):
        _execution_device = torch.device("cpu")

        def decode_latents(self, latents, inter=None):
            return np.zeros((latents.shape[0], 32, 32, 3), dtype=np.float32)
    return Pipe(vae=_VAE(), text_encoder=None, tokenizer=None, unet=_UNet(), scheduler=scheduler)


def _cpu_args(**kw):
    a = dict(image=torch.zeros(2, 3, 32, 32), mask_image=torch.zeros(2, 1, 32, 32), pose_map=torch.zeros(2, 18, 32, 32),
             warped_cloth=torch.zeros(2, 3, 32, 32), prompt_embeds=torch.zeros(2, 4, 8), negative_prompt_embeds=torch.zeros(2, 4, 8),
             height=32, width=32, output_type="np", guidance_scale=1.0)
    a.update(kw)
    return a


@pytest.mark.parametrize("sched,eta,n,step_draws", [("lcm", 0.0, 1, 0), ("lcm", 0.0, 4, 3), ("tcd", 0.0, 4, 0), ("tcd", 0.3, 4, 3), ("tcd", 0.3, 1, 0)])
def test_modular_rng_contract(sched, eta, n, step_draws):
    """after the pipeline's three draws the modular step() draws one batch-shaped fp32 tensor at every evaluation but the last (TCD with
    eta = 0: none): the generator has advanced by exactly 3 + step_draws batch draws"""
    import ladi_vton_amd as L
    pipe = _cpu_pipe(L.LCMScheduler() if sched == "lcm" else L.TCDScheduler())
    g, gr = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    pipe(**_cpu_args(num_inference_steps=n, eta=eta, generator=g))
    for _ in range(3 + step_draws):
        torch.randn((2, 4, 4, 4), generator=gr, dtype=torch.float32)
    assert torch.equal(g.get_state(), gr.get_state())
    assert pipe.last_latents.shape == (2, 4, 4, 4) and bool(torch.isfinite(pipe.last_latents).all())


def test_surface():
    import ladi_vton_amd as L
    from ladi_vton_amd import pipeline as LP
    assert L.LCMScheduler().kind == LCM and L.TCDScheduler().kind == TCD
    assert L.LCMScheduler(original_inference_steps=100).kind == LCM | ORIG(100) and L.TCDScheduler(original_inference_steps=40).kind == TCD | ORIG(40)
    assert L.LCMScheduler in LP.FUSED_SCHEDULERS and L.TCDScheduler in LP.FUSED_SCHEDULERS
    assert L.LCMScheduler().config.timestep_scaling == 10.0
    with pytest.raises(NotImplementedError):
        L.LCMScheduler(timestep_scaling=5)
    with pytest.raises(ValueError):
        L.TCDScheduler(original_inference_steps=0)
    assert L.DDIMScheduler().kind == DDIM and L.DDIMScheduler().config.timestep_spacing == "leading"
    assert L.DDIMScheduler(timestep_spacing="trailing").kind == DDIM | TRAILING
    assert L.EulerDiscreteScheduler().kind == EULER and L.EulerDiscreteScheduler().config.timestep_spacing == "linspace"
    assert L.EulerDiscreteScheduler(timestep_spacing="trailing").kind == EULER | TRAILING
    assert L.EulerAncestralDiscreteScheduler(timestep_spacing="trailing").kind == EULER_A | TRAILING
    for cls, bad in ((L.DDIMScheduler, "linspace"), (L.EulerDiscreteScheduler, "leading"), (L.EulerAncestralDiscreteScheduler, "leading")):
        with pytest.raises(NotImplementedError):
            cls(timestep_spacing=bad)
    s = L.TCDScheduler()
    s.set_timesteps(4)
    with pytest.raises(ValueError):
        s.step(torch.zeros(1, 4, 2, 2), s.timesteps[0], torch.zeros(1, 4, 2, 2), eta=1.5)


@pytest.mark.parametrize("eta", [1.5, -0.1])
def test_pipeline_refuses_tcd_eta_outside_unit_interval_before_any_work(eta):
    import ladi_vton_amd as L

    class NoWork:
        config = _VAE.config

        def encode(self, x):
            raise AssertionError("work was done")
    pipe = _cpu_pipe(L.TCDScheduler())
    pipe.vae = NoWork()
    g = torch.Generator().manual_seed(1)
    before = g.get_state()
    with pytest.raises(ValueError, match="eta"):
        pipe(**_cpu_args(num_inference_steps=4, eta=eta, generator=g))
    assert torch.equal(g.get_state(), before)
