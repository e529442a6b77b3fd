"""Reference for the guidance schedule, the CFG cut-off and guidance rescale: the yardstick tests/test_cpu_guidance.py and
tests/test_gpu_guidance.py compare the library with.  float64 torch for the statistics; nothing here imports the package under test.  The
try-on loop that applies the combine per evaluation is tests/ref_tryon.py's (table=, phi=).

    e_i = u + g_i (c - u)                                   for a CFG evaluation (g_i > 1)
    e_i = e_i * (phi * std(c) / std(e_i) + (1 - phi))       guidance rescale, per sample over all its elements, torch.std's default
                                                            (unbiased) correction, no epsilon
    e_i = c                                                 for a cond-only evaluation (g_i <= 1): the unconditional half is not evaluated,
                                                            the rule tryon_pipe.py applies to a whole run (do_classifier_free_guidance)
"""


def is_cfg(g):
    return g > 1.0


def rescale_factor(e, ec, phi):
    """[n, 1, ...] float64: phi * std(ec) / std(e) + (1 - phi) per sample"""
    dims = list(range(1, e.ndim))
    return phi * (ec.double().std(dim=dims, keepdim=True) / e.double().std(dim=dims, keepdim=True)) + (1.0 - phi)


def guided_eps(eu, ec, g, phi=0.0):
    """eu, ec: [n, ...] unconditional / conditional predictions.  The combine runs in the inputs' dtype (float64 inputs: all float64; the fp32
    oracle's tensors: the oracle's own arithmetic, so phi = 0 restates it exactly), the rescale statistics always in float64"""
    e = eu + g * (ec - eu)
    if phi > 0.0:
        e = (e.double() * rescale_factor(e, ec, phi)).to(e.dtype)
    return e


def sched_reference(sch, eps_seq, table, phi, lat0, generator=None):
    """the loop of test_scheduler_ext_device_vs_mirror with the per-evaluation combine.  sch: a scheduler mirror with set_timesteps done;
    eps_seq: [evals, 2B, 4, h, w] ([uncond ; cond] per evaluation; the uncond half of a cond-only evaluation is never touched, it may hold
    NaN); table: one scale per evaluation; lat0 [B, 4, h, w]; generator: for the schedulers whose step() draws noise"""
    B = lat0.shape[0]
    x = lat0.double()
    extra = {} if generator is None else {"generator": generator}
    assert len(table) == len(sch.timesteps) == eps_seq.shape[0]
    for i, t in enumerate(sch.timesteps):
        ec = eps_seq[i, B:].double()
        e = guided_eps(eps_seq[i, :B].double(), ec, table[i], phi) if is_cfg(table[i]) else ec
        x = sch.step(e, t, x, **extra).prev_sample
    return x
