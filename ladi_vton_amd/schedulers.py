"""Host-side mirrors of the three schedulers the reference pipeline accepts (tryon_pipe.py:62: diffusers 0.14.0 DDIMScheduler — what
src/inference.py:123-124 instantiates —, PNDMScheduler with skip_prk_steps, which the SD2-inpainting scheduler_config.json
describes, and LMSDiscreteScheduler).  They expose the attributes tryon_pipe.py touches
(:74,88,331-346,424,650-651,711,722,740).

Three more diffusers 0.14.0 schedulers work as the reference pipeline's `scheduler` because it only calls set_timesteps,
scale_model_input, step, timesteps, init_noise_sigma and order: DPMSolverMultistepScheduler (dpmsolver++), EulerDiscreteScheduler and
EulerAncestralDiscreteScheduler, mirrored here with the same SD2-inpainting config (scaled_linear 0.00085-0.012, 1000 training steps,
epsilon prediction).  Their formulas are restated from the published algorithms as diffusers 0.14 ships them, from memory: diffusers is
not installable here, so they are not pinned against it (like the other three).

Few-step sampling of distilled weights: LCMScheduler and TCDScheduler (1 .. original_inference_steps evaluations), and
timestep_spacing="trailing" on DDIMScheduler, EulerDiscreteScheduler and EulerAncestralDiscreteScheduler (1 .. 1000), restated the same way;
the scheduler block of include/ladi_native.h is the contract for their timesteps and updates.

The fused native loop (ladi_tryon_run) does not call .step(): it consumes the same tables on the device.  .step() here serves
the module-by-module drop-in path and operates on small [B,4,h,w] tensors.
"""
import math
from types import SimpleNamespace

import torch

from . import _lib

DDIM, PNDM, LMS, DPMPP, EULER, EULER_ANCESTRAL = 0, 1, 2, 3, 4, 5
LCM, TCD = 7, 8
# option bits of the scheduler code (include/ladi_native.h): bit 6 trailing timestep spacing (DDIM, Euler, Euler-ancestral), bits 12-21
# original_inference_steps of LCM / TCD (0 = 50)
TRAILING = 1 << 6


def _spacing_bit(cls_name, timestep_spacing, default):
    """timestep_spacing of DDIM / Euler / Euler-ancestral: the class's diffusers default or "trailing" (Turbo, Lightning, Hyper-SD weights)"""
    if timestep_spacing == default:
        return 0
    if timestep_spacing == "trailing":
        return TRAILING
    raise NotImplementedError("%s: timestep_spacing=%r is not implemented (only %r, the default, and 'trailing')"
                              % (cls_name, timestep_spacing, default))


def _alphas_cumprod():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


class _SchedulerBase:
    order = 1
    init_noise_sigma = 1.0
    kind = None

    def __init__(self):
        self.alphas_cumprod = _alphas_cumprod()
        self.final_alpha_cumprod = self.alphas_cumprod[0]  # set_alpha_to_one = False
        self.config = SimpleNamespace(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                      steps_offset=1, skip_prk_steps=True, set_alpha_to_one=False, clip_sample=False,
                                      prediction_type="epsilon")
        self.timesteps = None
        self.num_inference_steps = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _native_timesteps(self, n):
        import ctypes
        buf = (ctypes.c_int * (n + 2))()
        cnt = _lib.load().ladi_sched_timesteps(self.kind, n, buf, n + 2)
        if cnt < 0:
            raise _lib.NativeError("ladi_sched_timesteps: " + _lib.last_error())
        return list(buf[:cnt])

    def _a(self, t):
        return self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod

    def _check_first_step(self, n, first_step, min_tail=1):
        """strength: the run starts at step first_step of the n-step schedule; the tail keeps at least min_tail steps"""
        first_step = int(first_step)
        if first_step < 0 or first_step > int(n) - min_tail:
            raise ValueError("first_step %d is out of range [0, %d] for %d steps%s"
                             % (first_step, int(n) - min_tail, int(n), " (a PNDM tail needs at least 2 steps)" if min_tail == 2 else ""))
        return first_step

    def _native_table_from(self, n, first_step):
        """-> (timesteps, rows [evals][10], (k_x, k_n, in_scale0)) of ladi_sched_table_from: the very numbers the fused loop uses for the tail"""
        import ctypes
        ts, rows, start = (ctypes.c_double * (n + 2))(), (ctypes.c_float * (10 * (n + 2)))(), (ctypes.c_float * 3)()
        ac = self.alphas_cumprod.to("cpu", torch.float32).contiguous()
        cnt = _lib.load().ladi_sched_table_from(self.kind, n, ctypes.c_void_p(ac.data_ptr()), 0.0, first_step, ts, rows, n + 2, start)
        if cnt < 0:
            raise _lib.NativeError("ladi_sched_table_from: " + _lib.last_error())
        return list(ts[:cnt]), [list(rows[10 * i:10 * i + 10]) for i in range(cnt)], tuple(start)

    def add_noise(self, original_samples, noise, timesteps):
        """sqrt(a_t) x0 + sqrt(1 - a_t) noise at the integer timestep t (diffusers' add_noise; coefficients in float64)"""
        a = float(self.alphas_cumprod[int(timesteps)].double())
        return (a ** 0.5 * original_samples.double() + (1.0 - a) ** 0.5 * noise.double()).to(original_samples.dtype)


def _step_noise(shape, dtype, generator, device):
    """diffusers 0.14 randn_tensor(shape, generator, device, dtype) as the schedulers' step() calls it: drawn on the generator's device;
    a LIST of generators draws one [1, ...] tensor per sample from that sample's generator"""
    if isinstance(generator, (list, tuple)):
        if len(generator) != shape[0]:
            raise ValueError("You have passed a list of generators of length %d, but requested an effective batch size of %d."
                             % (len(generator), shape[0]))
        return torch.cat([torch.randn((1,) + shape[1:], generator=g_, device=g_.device, dtype=dtype).to(device) for g_ in generator], dim=0)
    gdev = generator.device if generator is not None else device
    return torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)


class DDIMScheduler(_SchedulerBase):
    """timestep_spacing="trailing": t_i = round_half_even(1000 - i * (1000 / n)) - 1 and, as in diffusers, prev = t - 1000 // n (n = 3: 666,
    333, -1: not the next timestep); one step is allowed then (the default "leading" keeps n >= 2)"""
    kind = DDIM

    def __init__(self, timestep_spacing="leading"):
        super().__init__()
        self.kind = DDIM | _spacing_bit("DDIMScheduler", timestep_spacing, "leading")
        self.config.timestep_spacing = timestep_spacing

    def set_timesteps(self, num_inference_steps, device=None, first_step=0):
        """first_step > 0 (strength): the timesteps of steps first_step .. of the schedule"""
        first_step = self._check_first_step(num_inference_steps, first_step)
        self.num_inference_steps = num_inference_steps
        self.ratio = 1000 // num_inference_steps
        ts = self._native_timesteps(num_inference_steps)[first_step:]
        self.timesteps = torch.tensor(ts, dtype=torch.int64, device=device)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None, variance_noise=None, **kw):
        """DDIM eq. (12) as diffusers 0.14 writes it: sigma_t = eta * sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)); the stochastic
        term (eta > 0) draws ONE batch-shaped normal tensor from `generator` per step (randn_tensor), or uses `variance_noise`"""
        t = int(timestep)
        a_t, a_p = float(self._a(t)), float(self._a(t - self.ratio))
        x, e = sample.float(), model_output.float()
        x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
        var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        std = float(eta) * max(var, 0.0) ** 0.5
        prev = a_p ** 0.5 * x0 + max(1 - a_p - std * std, 0.0) ** 0.5 * e
        if use_clipped_model_output:
            raise NotImplementedError("use_clipped_model_output=True is not implemented (the try-on pipeline never sets it: tryon_pipe.py:740)")
        if eta > 0:
            if variance_noise is None:
                # randn_tensor(model_output.shape, generator, device, dtype=model_output.dtype)
                variance_noise = _step_noise(tuple(model_output.shape), model_output.dtype, generator, sample.device)
            prev = prev + std * variance_noise.float()
        return SimpleNamespace(prev_sample=prev.to(sample.dtype))


class PNDMScheduler(_SchedulerBase):
    kind = PNDM

    def set_timesteps(self, num_inference_steps, device=None, first_step=0):
        """first_step > 0 (strength): a fresh PLMS run over the step timesteps u0 > u1 > .. of steps first_step .., evaluations
        [u0, u1, u1, u2, ..] (tail steps + 1) -- not diffusers' slice of the N + 1 list, which leaves the sample one step under-denoised.
        The tail needs at least 2 steps."""
        first_step = self._check_first_step(num_inference_steps, first_step, min_tail=2 if first_step else 1)
        self.num_inference_steps = num_inference_steps
        self.ratio = 1000 // num_inference_steps
        ts = self._native_timesteps(num_inference_steps)
        if first_step:
            u = ([ts[0]] + ts[2:])[first_step:]          # the schedule's step timesteps, then the tail's
            ts = [u[0], u[1], u[1]] + u[2:]
        self.timesteps = torch.tensor(ts, dtype=torch.int64, device=device)
        self.ets, self.counter, self.cur_sample = [], 0, None

    def step(self, model_output, timestep, sample, **kw):
        t = int(timestep)
        tp = t - self.ratio
        e_now, x = model_output.float(), sample.float()
        if self.counter != 1:
            self.ets = self.ets[-3:] + [e_now]
        else:
            tp, t = t, t + self.ratio
        n = len(self.ets)
        if n == 1 and self.counter == 0:
            e, self.cur_sample = e_now, x
        elif n == 1 and self.counter == 1:
            e, x, self.cur_sample = (e_now + self.ets[-1]) / 2, self.cur_sample, None
        elif n == 2:
            e = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif n == 3:
            e = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            e = (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4]) / 24
        a_t, a_p = float(self._a(t)), float(self._a(tp))
        denom = a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5
        prev = (a_p / a_t) ** 0.5 * x - (a_p - a_t) * e / denom
        self.counter += 1
        return SimpleNamespace(prev_sample=prev.to(sample.dtype))


class DPMSolverMultistepScheduler(_SchedulerBase):
    """diffusers 0.14 DPMSolverMultistepScheduler with algorithm_type="dpmsolver++" (DPM-Solver++ 2M by default), epsilon prediction.

    Restated from memory (not pinned against diffusers): timesteps linspace(0, 999, n + 1).round()[::-1][:-1] (round half to even; the
    native builder refuses n whose timesteps repeat, e.g. n = 1000, on which diffusers fails in step()); alpha = sqrt(a), sigma =
    sqrt(1 - a), lambda = log(alpha) - log(sigma); data prediction m = (x - sigma_s eps) / alpha_s; prev_t = 0 at the last step; with
    h = lambda_t - lambda_s0, r0 = h_0 / h, r1 = h_1 / h:
      first order : x_t = (sigma_t / sigma_s) x - alpha_t (e^-h - 1) m0
      second order: D1 = (m0 - m1) / r0; midpoint adds -0.5 alpha_t (e^-h - 1) D1, heun adds alpha_t ((e^-h - 1) / h + 1) D1
      third order : D1_0 = (m0 - m1) / r0, D1_1 = (m1 - m2) / r1, D1 = D1_0 + r0 / (r0 + r1) (D1_0 - D1_1), D2 = (D1_0 - D1_1) / (r0 + r1);
                    x_t = (sigma_t / sigma_s0) x - alpha_t (e^-h - 1) m0 + alpha_t ((e^-h - 1) / h + 1) D1 - alpha_t ((e^-h - 1 + h) / h^2 - 0.5) D2
    Warm-up: first order at the first step, at most second at the second; lower_order_final (only if n < 15): first order at the last
    step, at most second at the one before.  The fused device loop uses the native table (mode 2 of the step kernel: the history ring holds
    the data predictions)."""

    def __init__(self, solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, thresholding=False,
                 prediction_type="epsilon"):
        if solver_order not in (1, 2, 3):
            raise ValueError("solver_order must be 1, 2 or 3, got %r" % (solver_order,))
        if solver_type not in ("midpoint", "heun"):
            raise ValueError("solver_type must be 'midpoint' or 'heun', got %r" % (solver_type,))
        if algorithm_type != "dpmsolver++":
            raise NotImplementedError("DPMSolverMultistepScheduler: only algorithm_type='dpmsolver++' is implemented, got %r" % (algorithm_type,))
        if thresholding:
            raise NotImplementedError("DPMSolverMultistepScheduler: thresholding=True is not implemented")
        if prediction_type != "epsilon":
            raise NotImplementedError("DPMSolverMultistepScheduler: only prediction_type='epsilon' is implemented, got %r" % (prediction_type,))
        super().__init__()
        self.config.solver_order, self.config.algorithm_type, self.config.solver_type = solver_order, algorithm_type, solver_type
        self.config.lower_order_final, self.config.thresholding = bool(lower_order_final), False
        # scheduler code (include/ladi_native.h): kind 3, bits 8-9 solver_order (0 = 2), bit 10 heun, bit 11 lower_order_final off
        self.kind = (DPMPP | ((solver_order if solver_order != 2 else 0) << 8) | ((solver_type == "heun") << 10)
                     | ((not lower_order_final) << 11))
        ac = self.alphas_cumprod.double()
        self.alpha_t, self.sigma_t = ac.sqrt(), (1 - ac).sqrt()
        self.lambda_t = self.alpha_t.log() - self.sigma_t.log()

    def set_timesteps(self, num_inference_steps, device=None, first_step=0):
        """first_step > 0 (strength): steps first_step .. of the schedule; the solver warms up again there (no earlier data predictions) and
        lower_order_final acts where it does in the whole run"""
        n = int(num_inference_steps)
        first_step = self._check_first_step(n, first_step)
        self.num_inference_steps = n
        self._ts = self._native_timesteps(n)[first_step:]
        self.timesteps = torch.tensor(self._ts, dtype=torch.int64, device=device)
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0

    def _coef(self, t):
        return float(self.alpha_t[t]), float(self.sigma_t[t]), float(self.lambda_t[t])

    def step(self, model_output, timestep, sample, return_dict=True, **kw):
        t_s = int(timestep)
        ts, n, order = self._ts, len(self._ts), self.config.solver_order
        i = ts.index(t_s) if t_s in ts else n - 1
        prev_t = 0 if i == n - 1 else ts[i + 1]
        lof = self.config.lower_order_final and self.num_inference_steps < 15
        x, e = sample.float(), model_output.float()
        a_s, s_s, l_s = self._coef(t_s)
        m = (x - s_s * e) / a_s
        self.model_outputs = self.model_outputs[1:] + [m]
        a_t, s_t, l_t = self._coef(prev_t)
        h = l_t - l_s
        em = math.expm1(-h)
        prev = (s_t / s_s) * x - a_t * em * m
        if not (order == 1 or self.lower_order_nums < 1 or (lof and i == n - 1)):
            m0, m1 = self.model_outputs[-1], self.model_outputs[-2]
            r0 = (l_s - self._coef(ts[i - 1])[2]) / h
            if order == 2 or self.lower_order_nums < 2 or (lof and i == n - 2):
                d1 = (m0 - m1) / r0
                if self.config.solver_type == "midpoint":
                    prev = prev - 0.5 * a_t * em * d1
                else:
                    prev = prev + a_t * (em / h + 1.0) * d1
            else:
                m2 = self.model_outputs[-3]
                r1 = (self._coef(ts[i - 1])[2] - self._coef(ts[i - 2])[2]) / h
                d1_0, d1_1 = (m0 - m1) / r0, (m1 - m2) / r1
                d1 = d1_0 + (r0 / (r0 + r1)) * (d1_0 - d1_1)
                d2 = (d1_0 - d1_1) / (r0 + r1)
                prev = prev + a_t * (em / h + 1.0) * d1 - a_t * ((em + h) / (h * h) - 0.5) * d2
        if self.lower_order_nums < order:
            self.lower_order_nums += 1
        return SimpleNamespace(prev_sample=prev.to(sample.dtype))


class _SigmaScheduler(_SchedulerBase):
    """the sigma parameterisation LMSDiscrete, EulerDiscrete and EulerAncestralDiscrete share: fractional timesteps
    linspace(0, 999, n)[::-1], sigmas interpolated from sqrt((1 - a) / a) in fp32 with a trailing 0, init_noise_sigma = max sigma,
    scale_model_input = sample / sqrt(sigma^2 + 1).  The tables come from the native builder (ladi_sched_lms), i.e. they are the very
    numbers the fused device loop uses."""

    def __init__(self, timestep_spacing="linspace"):
        super().__init__()
        self.kind = type(self).kind | _spacing_bit(type(self).__name__, timestep_spacing, "linspace")
        self.config.timestep_spacing = timestep_spacing
        self.sigmas = None
        self.init_noise_sigma = float(((1 - self.alphas_cumprod) / self.alphas_cumprod).sqrt().max())   # as diffusers before set_timesteps

    def _set_sigma_tables(self, num_inference_steps, device, first_step=0):
        import ctypes
        n = int(num_inference_steps)
        first_step = self._check_first_step(n, first_step)
        if self.kind & TRAILING:
            # timestep_spacing="trailing": integer timesteps t_i = round_half_even(1000 - i * (1000 / n)) - 1 from the native builder,
            # sigma = sqrt((1 - a) / a) at them in float64, held in fp32 (the builder's arithmetic), trailing 0; one step is allowed
            tl = self._native_timesteps(n)
            ac = [float(self.alphas_cumprod[t]) for t in tl]
            sg = [float(torch.tensor(math.sqrt((1.0 - a) / a), dtype=torch.float32)) for a in ac] + [0.0]
            self.num_inference_steps = n
            self.timesteps = torch.tensor([float(t) for t in tl][first_step:], dtype=torch.float64, device=device)
            self.sigmas = torch.tensor(sg[first_step:], dtype=torch.float32)
            self._ts = [float(t) for t in tl][first_step:]
            self.init_noise_sigma = float(max(sg))
            return None
        ts = (ctypes.c_double * n)()
        sg = (ctypes.c_float * (n + 1))()
        cf = (ctypes.c_float * (4 * n))()
        ac = self.alphas_cumprod.to("cpu", torch.float32).contiguous()      # the same table the fused loop receives
        if _lib.load().ladi_sched_lms(n, ctypes.c_void_p(ac.data_ptr()), ts, sg, cf) < 0:
            raise _lib.NativeError("ladi_sched_lms: " + _lib.last_error())
        self.num_inference_steps = n
        # first_step > 0 (strength): the timesteps and sigmas of steps first_step ..; init_noise_sigma stays the whole schedule's
        self.timesteps = torch.tensor(list(ts)[first_step:], dtype=torch.float64, device=device)
        self.sigmas = torch.tensor(list(sg)[first_step:], dtype=torch.float32)
        self._ts = list(ts)[first_step:]
        self.init_noise_sigma = float(max(sg))
        return cf

    def add_noise(self, original_samples, noise, timesteps):
        """x0 + sigma_t noise (diffusers' add_noise of the sigma schedulers)"""
        sigma = float(self.sigmas[self._index(timesteps)])
        return (original_samples.double() + sigma * noise.double()).to(original_samples.dtype)

    def _index(self, timestep):
        t = float(timestep)
        return min(range(len(self._ts)), key=lambda i: abs(self._ts[i] - t))

    def scale_model_input(self, sample, timestep=None):
        sigma = float(self.sigmas[self._index(timestep)])
        return sample / ((sigma * sigma + 1.0) ** 0.5)


class EulerDiscreteScheduler(_SigmaScheduler):
    """diffusers 0.14 EulerDiscreteScheduler, epsilon prediction, s_churn = 0 only: prev = x + (sigma_{i+1} - sigma_i) eps.  Like diffusers,
    step() draws one noise tensor per call even without churn (it is unused), so a generator ends a run in the reference's state.
    Restated from memory, not pinned against diffusers."""
    kind = EULER

    def set_timesteps(self, num_inference_steps, device=None, first_step=0):
        self._set_sigma_tables(num_inference_steps, device, first_step)

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None,
             return_dict=True, **kw):
        if s_churn != 0:
            raise NotImplementedError("EulerDiscreteScheduler.step: only s_churn = 0 is implemented")
        i = self._index(timestep)
        x, e = sample.float(), model_output.float()
        _step_noise(tuple(model_output.shape), torch.float32, generator, sample.device)
        prev = x + (float(self.sigmas[i + 1]) - float(self.sigmas[i])) * e
        return SimpleNamespace(prev_sample=prev.to(sample.dtype))


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """diffusers 0.14 EulerAncestralDiscreteScheduler, epsilon prediction: sigma_up = sqrt(s_to^2 (s_from^2 - s_to^2) / s_from^2),
    sigma_down = sqrt(s_to^2 - sigma_up^2), prev = x + (sigma_down - sigma) eps + sigma_up noise, one fp32 noise tensor drawn per step
    (on the generator's device; a LIST of generators draws one [1, ...] tensor per sample).  The fused loop takes the same draws,
    made up front in the same generator order (ladi_tryon_set_step_noise).  Restated from memory, not pinned against diffusers."""
    kind = EULER_ANCESTRAL

    def set_timesteps(self, num_inference_steps, device=None, first_step=0):
        self._set_sigma_tables(num_inference_steps, device, first_step)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, **kw):
        i = self._index(timestep)
        s_from, s_to = float(self.sigmas[i]), float(self.sigmas[i + 1])
        up = (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5
        down = max(s_to ** 2 - up ** 2, 0.0) ** 0.5
        x, e = sample.float(), model_output.float()
        noise = _step_noise(tuple(model_output.shape), torch.float32, generator, sample.device)
        prev = x + (down - s_from) * e + up * noise
        return SimpleNamespace(prev_sample=prev.to(sample.dtype))


class LMSDiscreteScheduler(_SigmaScheduler):
    """diffusers 0.14 LMSDiscreteScheduler (order-4 linear multistep in the sigma parameterisation, epsilon prediction).  The
    fractional timesteps, the sigmas and the multistep weights all come from the native table builder (ladi_sched_lms), i.e. they
    are the very numbers the fused device loop uses."""
    kind = LMS

    def __init__(self):
        super().__init__()      # (no timestep_spacing: trailing spacing is DDIM, Euler and Euler-ancestral only)

    def set_timesteps(self, num_inference_steps, device=None, first_step=0):
        """first_step > 0 (strength): steps first_step .. with the multistep weights of a history that starts empty there (orders 1, 2, ..)"""
        cf = self._set_sigma_tables(num_inference_steps, device, first_step)
        if first_step:
            self._coeffs = [row[2:6] for row in self._native_table_from(self.num_inference_steps, int(first_step))[1]]
        else:
            self._coeffs = [list(cf[4 * i:4 * i + 4]) for i in range(self.num_inference_steps)]
        self.derivatives = []

    def step(self, model_output, timestep, sample, order=4, **kw):
        if order != 4:
            raise NotImplementedError("LMSDiscreteScheduler.step: only the default order = 4 is supported")
        i = self._index(timestep)
        sigma = float(self.sigmas[i])
        x, e = sample.float(), model_output.float()
        x0 = x - sigma * e
        self.derivatives = (self.derivatives + [(x - x0) / sigma])[-4:]
        prev = x
        for c, d in zip(self._coeffs[i][:min(i + 1, 4)], reversed(self.derivatives)):
            prev = prev + c * d
        return SimpleNamespace(prev_sample=prev.to(sample.dtype))


class _FewStepScheduler(_SchedulerBase):
    """what LCMScheduler and TCDScheduler share: the timesteps of a distilled model.  With O = original_inference_steps and k = 1000 // O,
    t_i = (O - floor(i * (O / n))) * k - 1, i * (O / n) evaluated as numpy.linspace(0, O, n, endpoint=False) does (O = 50, n = 4: 999, 759,
    499, 259); 1 <= n <= O.  They come from the native builder (ladi_sched_timesteps), i.e. they are the fused loop's.  first_step > 0
    (strength) runs the tail of the n-step list like every other scheduler here -- not diffusers' set_timesteps(strength=), which spaces
    the n steps anew over the shortened range.  Restated from the published algorithms as diffusers ships them, from memory: not pinned
    against diffusers."""
    _kind = None

    def __init__(self, original_inference_steps=50):
        o = int(original_inference_steps)
        if not 1 <= o <= 1000:
            raise ValueError("original_inference_steps must be in [1, 1000], got %r" % (original_inference_steps,))
        super().__init__()
        self.config.original_inference_steps = o
        # scheduler code (include/ladi_native.h): bits 12-21 original_inference_steps, 0 = the default 50
        self.kind = self._kind | ((o if o != 50 else 0) << 12)

    def set_timesteps(self, num_inference_steps, device=None, first_step=0):
        n = int(num_inference_steps)
        first_step = self._check_first_step(n, first_step)
        self.num_inference_steps = n
        self._ts = self._native_timesteps(n)[first_step:]
        self.timesteps = torch.tensor(self._ts, dtype=torch.int64, device=device)

    def _at(self, timestep):
        """-> (index of the timestep in this run, is it the last, a_t)"""
        t = int(timestep)
        i = self._ts.index(t)
        return i, i == len(self._ts) - 1, float(self.alphas_cumprod[t])


class LCMScheduler(_FewStepScheduler):
    """diffusers LCMScheduler (latent consistency models), epsilon prediction, timestep_scaling 10, sigma_data 0.5: with s = 10 t,
    c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25) and x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t), denoised = c_out x0 + c_skip x;
    every evaluation but the last returns sqrt(a_p) denoised + sqrt(1 - a_p) noise at a_p = alphas_cumprod[t_{i+1}] with one batch-shaped
    fp32 draw from `generator`, the last returns denoised and draws nothing.  The fused loop takes the same evaluations - 1 draws, made up
    front in the same generator order (ladi_tryon_set_step_noise; the last slab is zeros and never read)."""
    _kind = LCM

    def __init__(self, original_inference_steps=50, timestep_scaling=10.0):
        if float(timestep_scaling) != 10.0:
            raise NotImplementedError("LCMScheduler: only timestep_scaling = 10 is implemented, got %r" % (timestep_scaling,))
        super().__init__(original_inference_steps)
        self.config.timestep_scaling = 10.0

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, **kw):
        i, last, a_t = self._at(timestep)
        s = 10.0 * int(timestep)
        c_skip, c_out = 0.25 / (s * s + 0.25), s / math.sqrt(s * s + 0.25)
        x, e = sample.float(), model_output.float()
        x0 = (x - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
        denoised = c_out * x0 + c_skip * x
        prev = denoised
        if not last:
            a_p = float(self.alphas_cumprod[self._ts[i + 1]])
            noise = _step_noise(tuple(model_output.shape), torch.float32, generator, sample.device)
            prev = math.sqrt(a_p) * denoised + math.sqrt(1.0 - a_p) * noise
        return SimpleNamespace(prev_sample=prev.to(sample.dtype), denoised=denoised.to(sample.dtype))


class TCDScheduler(_FewStepScheduler):
    """diffusers TCDScheduler (trajectory consistency distillation), epsilon prediction; step()'s `eta` is the paper's gamma in [0, 1]:
    t_prev = t_{i+1} (0 after the last timestep), t_s = floor((1 - gamma) t_prev), x_s = sqrt(a_s) x0 + sqrt(1 - a_s) eps with
    x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t); with gamma > 0 every evaluation but the last returns sqrt(a_prev / a_s) x_s +
    sqrt(1 - a_prev / a_s) noise with one batch-shaped fp32 draw from `generator`; otherwise x_s, and nothing is drawn (gamma = 0 is a
    deterministic DDIM jump between the scheduler's own timesteps, the last one to t = 0).  The fused loop reads gamma from
    ladi_tryon_set_eta, in fp32 as the C ABI carries it: step() rounds it the same way."""
    _kind = TCD

    def step(self, model_output, timestep, sample, eta=0.3, generator=None, return_dict=True, **kw):
        gamma = float(torch.tensor(float(eta), dtype=torch.float32))
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("TCDScheduler.step: eta (gamma) has to be in [0, 1] but is %r." % (eta,))
        i, last, a_t = self._at(timestep)
        t_prev = 0 if last else self._ts[i + 1]
        t_s = int(math.floor((1.0 - gamma) * t_prev))
        a_s, a_prev = float(self.alphas_cumprod[t_s]), float(self.alphas_cumprod[t_prev])
        x, e = sample.float(), model_output.float()
        x0 = (x - math.sqrt(1.0 - a_t) * e) / math.sqrt(a_t)
        prev = math.sqrt(a_s) * x0 + math.sqrt(1.0 - a_s) * e
        if gamma > 0.0 and not last:
            noise = _step_noise(tuple(model_output.shape), torch.float32, generator, sample.device)
            prev = math.sqrt(a_prev / a_s) * prev + math.sqrt(max(1.0 - a_prev / a_s, 0.0)) * noise
        return SimpleNamespace(prev_sample=prev.to(sample.dtype), pred_noised_sample=prev.to(sample.dtype))
