"""CPU: the bounds that test_small_kernels_gpu.py holds air_adam_step to (tests/adam_oracle.py) admit the fp32 CPU
restatement of the step on the very inputs of those tests - the bounds rest on this, not on the kernel."""
import numpy as np

import adam_oracle as ao


def test_adam_bounds_admit_the_fp32_restatement():
    worst = np.zeros(3)
    for n, hyper, steps, moments in ao.adam_cases():
        p, _, m, v = ao.adam_inputs(n, 1, moments)
        for k in steps:
            g = ao.adam_inputs(n, k)[1]
            ref, tol = ao.adam_ref64(p, g, m, v, k, **hyper)
            got = ao.adam_restated32(p, g, m, v, k, **hyper)
            worst = np.maximum(worst, [ao.used(a, r, t) for a, r, t in zip(got, ref, tol)])
            ao.assert_adam(got, ref, tol, "fp32 restatement (n=%d, step %d, %s)" % (n, k, hyper))
            p, m, v = got
    print("fp32 restatement against fp64, largest fraction of the bound used: p %.3g, m %.3g, v %.3g" % tuple(worst))


def test_adam_bounds_are_the_plain_ones_where_nothing_cancels():
    """S = |g grad_scale| + |wd p| equals |g_eff| when both terms have one sign."""
    p = np.array([1.0, -2.0], np.float32)
    g = np.array([0.5, -0.25], np.float32)
    z = np.zeros(2, np.float32)
    (_, m1, v1), (_, tm, tv) = ao.adam_ref64(p, g, z, z, 1, **ao.ADAM_DEFAULT)
    b1, b2 = ao.f32(0.9), ao.f32(0.999)
    ge = m1 / (1.0 - b1)
    np.testing.assert_allclose(tm, ao.ADAM_CM * ao.EPS32 * np.abs((1.0 - b1) * ge), rtol=1e-12)
    np.testing.assert_allclose(tv, ao.ADAM_CV * ao.EPS32 * v1, rtol=1e-12)
