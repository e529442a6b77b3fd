"""Reference for the deep-feature cache (DeepCache on the full-resolution level): the plan, that is which evaluations run whole.  The forward
with its capture and shallow modes is tests/ref_unet.py's (cache=), the loop tests/ref_tryon.py's (feature_cache=); tests/test_cpu_feature_cache.py
and tests/test_gpu_feature_cache.py compare the library with them.

    plan                     one flag per evaluation, True = whole; flag 0 is whole.  Promotion: in a CFG-shaped run a shallow evaluation over
                             all 2B samples whose most recent whole evaluation ran cond-only (and so refreshed the conditional rows only) runs
                             whole; a shallow cond-only evaluation never does
"""


def plan(n_evals, interval, cond_only=None):
    """-> [bool] * n_evals after promotion.  interval: an int N >= 1 (whole at i % N == 0) or a sequence of n_evals flags; cond_only: None or
    one flag per evaluation (True: that evaluation of a CFG-shaped run runs over the conditional samples alone)"""
    flags = [i % interval == 0 for i in range(n_evals)] if isinstance(interval, int) else [bool(f) for f in interval]
    assert len(flags) == n_evals
    co = [False] * n_evals if cond_only is None else [bool(c) for c in cond_only]
    if flags:
        flags[0] = True
    only_cond_rows_fresh = False
    for i in range(n_evals):
        if not flags[i] and not co[i] and only_cond_rows_fresh:
            flags[i] = True
        if flags[i]:
            only_cond_rows_fresh = co[i]
    return flags
