"""GPU: the dispatcher's guard on handles of two dtypes (csrc/mhx_abi.cpp, NEED_SAME).  A target built on a context of the other
dtype is refused by every entry point that takes a context and a target -- MHX_EINVAL, "different dtype", *out untouched -- before
either engine sees a handle that is not its own; afterwards both contexts create and sample as before."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_a_target_of_the_other_dtype_is_refused(mhx, real):
    L = mhx._lib
    other = {"f32": "f64", "f64": "f32"}[real]
    ctx, octx = mhx.Context.default(dtype=real), mhx.Context.default(dtype=other)
    model = mhx.DensityModel(mhx.IsoGaussian(2))
    t = model.handle(octx)                                     # the target lives on the context of the OTHER dtype
    lib = mhx.lib()
    rw = L.RwmhCfg(2, 8, 1, 0, L.PROP_ISO, 1.0, None, 0, None, 0)
    em = L.EmceeCfg(2, 8, 1, 0, 2.0, 0, 0, 0, 1.0, None, None, 1)
    ram = L.RamCfg(2, 8, 1, 0, 0.234, 0.6, 0.0, float("inf"), 0)
    mala = L.MalaCfg(2, 8, 1, 0, 0.5, 0, 0)
    x, lp = ctx.arr(np.zeros((2, 1))), ctx.arr(np.full(1, 7.0))
    out = C.c_void_p()
    o = C.byref(out)
    calls = {
        "mhx_target_eval": lambda: lib.mhx_target_eval(ctx.h, t, L.rptr(x), 1, L.rptr(lp)),
        "mhx_rwmh_create": lambda: lib.mhx_rwmh_create(ctx.h, t, C.byref(rw), o),
        "mhx_emcee_create": lambda: lib.mhx_emcee_create(ctx.h, t, C.byref(em), o),
        "mhx_ram_create": lambda: lib.mhx_ram_create(ctx.h, t, C.byref(ram), o),
        "mhx_mala_create": lambda: lib.mhx_mala_create(ctx.h, t, C.byref(mala), o),
        "mhx_rwmh_create_components": lambda: lib.mhx_rwmh_create_components(ctx.h, t, C.byref(rw), None, 0, o),
        "mhx_rwmh_create_conditional": lambda: lib.mhx_rwmh_create_conditional(ctx.h, t, C.byref(rw), None, 0, None, None, 0, o),
        "mhx_rwmh_create_composite": lambda: lib.mhx_rwmh_create_composite(ctx.h, t, C.byref(rw), None, 0, None, 0, None, None, None, 0, o),
    }
    for name, call in calls.items():
        assert call() == mhx.MHX_EINVAL, name
        msg = lib.mhx_last_error().decode()
        assert "different dtype" in msg and msg.startswith(name + ":"), (name, msg)
        assert not out.value, name
    assert lp[0] == 7.0                                        # mhx_target_eval wrote nothing
    # a same-dtype create on each context works afterwards
    for c in (ctx, octx):
        run = mhx.Run(model, mhx.RWMH(mhx.MvNormal(mhx.zeros(2), mhx.I)), nchains=8, seed=1, ctx=c)
        try:
            run.init(None)
            run.sample(3, 0, 1, 0)
            s = run.samples(False)[0]
            assert s.shape == (3, 3, 8) and s.dtype == c.real and np.isfinite(s).all()
        finally:
            run.close()
