// mhx_select.h -- the host side of the exact order statistics (include/mhx.h: mhx_*_order_statistics): the bucket scan that turns
// the integer histograms of one radix-select pass into the next key prefixes.  Pure host code, shared by both instantiations of
// the engine (a run histograms its own tensor) and by the group (the members' histograms are added first), so that one scan
// serves both.  The kernel is mhx_select_hist_body of mhx_diag_kernels.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

// digit width of a pass: the fewest passes (6 for fp64, 3 for fp32) and the fastest of the three measured;
// 8 and 10 bits are pre-built beside it for the comparison of tools/bench_quantiles.py (option SELECT_BITS)
#define MHX_SELECT_DIGIT_BITS 11
#define MHX_SELECT_MAX_DIGIT_BITS 11
// ranks served by one sequence of passes; more are processed in batches, so that the scratch (parameters x batch x bins
// counters) never grows with the number of ranks asked for
#define MHX_SELECT_BATCH 32

// One pass over one source of draws.  For parameter slot i, groups g < ngroups[i] with key prefix prefixes[i * gstride + g]
// (the bits above shift + digit_bits, right-aligned; shift + digit_bits == key width: the first pass, one group of all draws):
// hist[((i * gstride + g) << digit_bits) + b] = number of draws of that prefix whose digit (key >> shift) & (2^digit_bits - 1)
// is b.  Every counter of the groups in use is overwritten.
typedef int (*mhx_select_hist_fn)(void* user, const uint64_t* prefixes, const int32_t* ngroups, int32_t gstride, int32_t shift,
                                  int32_t digit_bits, uint64_t* hist);

// out[nparams][nranks] = the draws at the 0-based positions ranks[] of the ascending order of the S draws of every parameter
// slot; `who` names the entry point in messages.  Nothing is written to `out` unless the call succeeds.  `landing`: the caller's
// buffer for the histograms of a pass (what `fn` receives as `hist`), used when it holds at least mhx_select_hist_words() words --
// a context keeps a page-locked one from call to call; NULL or too small: pageable memory of the call.
int mhx_select_drive(const char* who, int keybits, int digit, int32_t nparams, const int64_t* ranks, int32_t nranks, uint64_t S,
                     mhx_select_hist_fn fn, void* user, double* out, uint64_t* landing, size_t landing_words);
// The key map of the device (mhx_order_key / mhx_key_value, mhx_device_math.h) on the host, for keys of `keybits` = 32 or 64 bits:
// the key of a value the select returned (a draw of that width, widened: the narrowing is exact), and the value of a key, where the
// all-ones key stands for every NaN.
uint64_t mhx_select_key_of(double v, int keybits);
double mhx_select_key_value(uint64_t k, int keybits);
// an upper bound of the words of `hist` a call with these arguments needs (0: the arguments are refused)
size_t mhx_select_hist_words(int digit, int32_t nparams, int32_t nranks);
