// launch_log.h -- a measurement build of libmhx.so that writes down what it asks the HIP runtime to launch.
//
//     make -C advancedmh.jl_amd/csrc EXTRA="-include $PWD/tools/launch_log.h" OUT=../libmhx_log.so
//     MHX_LAUNCH_LOG=launches.txt python tools/launch_shapes.py advancedmh.jl_amd/libmhx_log.so
//
// Force-included ahead of mhx_api.hip, it wraps the three ways that file launches a kernel -- hipLaunchKernelGGL,
// hipModuleLaunchKernel, hipLaunchKernel -- and appends one line per launch, in call order, to the file $MHX_LAUNCH_LOG names:
// `grid X Y block X lds BYTES`, the DYNAMIC LDS size of the call.  A kernel trace cannot show that number (rocprofv3's LDS column
// holds a kernel's static allocation only); tools/launch_trace.py joins this log to the trace.  The header knows nothing of the
// library's own code, so the same text instruments any commit of it: that is how two commits' launches are compared.  Host code
// only -- the device code of the objects does not change (tools/devcode_hash.sh).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

static inline void mhx_launch_log(dim3 grid, dim3 block, size_t lds)
{
    static FILE* f = getenv("MHX_LAUNCH_LOG") ? fopen(getenv("MHX_LAUNCH_LOG"), "a") : nullptr;
    if (!f) return;
    fprintf(f, "grid %u %u block %u lds %zu\n", grid.x, grid.y, block.x, lds);
    fflush(f);
}
static inline hipError_t mhx_logged_module_launch(hipFunction_t fn, unsigned gx, unsigned gy, unsigned gz, unsigned bx, unsigned by, unsigned bz,
                                                  unsigned lds, hipStream_t s, void** params, void** extra)
{
    mhx_launch_log(dim3(gx, gy, gz), dim3(bx, by, bz), lds);
    return hipModuleLaunchKernel(fn, gx, gy, gz, bx, by, bz, lds, s, params, extra);
}
static inline hipError_t mhx_logged_launch(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t s)
{
    mhx_launch_log(grid, block, lds);
    return hipLaunchKernel(fn, grid, block, args, lds, s);
}
#define hipModuleLaunchKernel mhx_logged_module_launch
#define hipLaunchKernel mhx_logged_launch
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, numBlocks, numThreads, memPerBlock, streamId, ...)            \
    do {                                                                                              \
        mhx_launch_log(dim3(numBlocks), dim3(numThreads), (size_t)(memPerBlock));                     \
        (kernelName)<<<(numBlocks), (numThreads), (memPerBlock), (streamId)>>>(__VA_ARGS__);          \
    } while (0)
