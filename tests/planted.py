"""A run whose device sample buffer holds a crafted tensor: what the GPU tests of the post-run statistics compute on."""
import ctypes as C

import numpy as np


def plant_ptr(mhx, x):
    """(run, device pointer): a run whose device sample buffer holds x [N][dim+1][C] (mhx_run_device_samples hands out the pointer),
    read back and compared bit for bit"""
    N, d1, nch = x.shape
    d = d1 - 1
    run = mhx.Run(mhx.DensityModel(mhx.IsoGaussian(d)), mhx.RWMH(mhx.MvNormal(mhx.zeros(d), mhx.I)), nchains=nch, seed=1)
    run.init(None)
    run.sample(N, 0, 1, 0)
    assert x.dtype == run.real and x.flags.c_contiguous
    ptr, n = C.c_void_p(), C.c_int64()
    mhx.check(mhx.lib().mhx_run_device_samples(run.h, C.byref(ptr), None, C.byref(n)))
    assert n.value == N and ptr.value
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(ptr, x.ctypes.data_as(C.c_void_p), x.nbytes, 1) == 0        # hipMemcpyHostToDevice, blocking
    back, _ = run.samples(want_accepted=False)
    assert np.array_equal(back.view(np.uint8), x.view(np.uint8))
    return run, ptr


def plant(mhx, x):
    """the run of plant_ptr alone"""
    return plant_ptr(mhx, x)[0]
