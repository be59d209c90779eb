// mhx_select.cpp -- bucket scan and pass loop of the exact order statistics (mhx_select.h).  No HIP here.
#include "mhx_select.h"

#include "mhx_impl.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

uint64_t mhx_select_key_of(double v, int keybits)
{
    if (v != v) return ~0ull;
    if (keybits == 64) {
        uint64_t b;
        memcpy(&b, &v, sizeof b);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
    const float f = (float)v;
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return (uint64_t)((b >> 31) ? ~b : (b | 0x80000000u));
}

double mhx_select_key_value(uint64_t k, int keybits)
{
    if (keybits == 64) {
        if (k == ~0ull) return std::nan("");
        const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
        double x;
        memcpy(&x, &b, sizeof x);
        return x;
    }
    const uint32_t k32 = (uint32_t)k;
    if (k32 == ~0u) return std::nan("");
    const uint32_t b = (k32 >> 31) ? (k32 ^ 0x80000000u) : ~k32;
    float x;
    memcpy(&x, &b, sizeof x);
    return (double)x;                                      // exact
}

size_t mhx_select_hist_words(int digit, int32_t nparams, int32_t nranks)
{
    if (digit < 1 || digit > MHX_SELECT_MAX_DIGIT_BITS || nparams <= 0 || nranks <= 0) return 0;
    return ((size_t)nparams * std::min<size_t>((size_t)nranks, MHX_SELECT_BATCH)) << digit;
}

int mhx_select_drive(const char* who, int keybits, int digit, int32_t nparams, const int64_t* ranks, int32_t nranks, uint64_t S,
                     mhx_select_hist_fn fn, void* user, double* out, uint64_t* landing, size_t landing_words)
{
    if (nparams <= 0 || nranks <= 0 || !ranks || !out) return mhx_fail(MHX_EINVAL, "%s: bad argument", who);
    if (digit < 1 || digit > MHX_SELECT_MAX_DIGIT_BITS) return mhx_fail(MHX_EINVAL, "%s: digit width %d outside [1, %d]", who, digit, MHX_SELECT_MAX_DIGIT_BITS);
    for (int32_t j = 0; j < nranks; ++j)
        if (ranks[j] < 0 || (uint64_t)ranks[j] >= S)
            return mhx_fail(MHX_EINVAL, "%s: rank %lld outside [0, %llu)", who, (long long)ranks[j], (unsigned long long)S);
    // distinct ranks in ascending order: neighbours share prefixes longest, and a repeated rank costs nothing
    std::vector<uint64_t> u(ranks, ranks + nranks);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    const size_t T = u.size();
    const int32_t gstride = (int32_t)std::min<size_t>(T, MHX_SELECT_BATCH);
    const size_t nhist = ((size_t)nparams * gstride) << digit;
    std::vector<uint64_t> own;
    if (!landing || landing_words < nhist) { own.resize(nhist); landing = own.data(); }
    uint64_t* hist = landing;
    std::vector<double> res((size_t)nparams * T);
    std::vector<uint64_t> prefix((size_t)nparams * gstride), next_prefix(gstride), resid((size_t)nparams * gstride);
    std::vector<int32_t> ngroups(nparams), grp((size_t)nparams * gstride);
    for (size_t b0 = 0; b0 < T; b0 += MHX_SELECT_BATCH) {
        const int nt = (int)std::min<size_t>(MHX_SELECT_BATCH, T - b0);
        for (int32_t p = 0; p < nparams; ++p) {
            ngroups[p] = 1;
            prefix[(size_t)p * gstride] = 0;
            for (int k = 0; k < nt; ++k) { grp[(size_t)p * gstride + k] = 0; resid[(size_t)p * gstride + k] = u[b0 + k]; }
        }
        for (int remaining = keybits; remaining > 0;) {
            const int db = std::min(digit, remaining), shift = remaining - db;
            const int rc = fn(user, prefix.data(), ngroups.data(), gstride, shift, db, hist);
            if (rc) return rc;
            const uint64_t nb = 1ull << db;
            for (int32_t p = 0; p < nparams; ++p) {
                int32_t* g_of = grp.data() + (size_t)p * gstride;
                uint64_t* r_of = resid.data() + (size_t)p * gstride;
                uint64_t* pf = prefix.data() + (size_t)p * gstride;
                int32_t nng = 0;
                for (int k = 0; k < nt;) {
                    // the targets of one group are neighbours with ascending residual ranks: one walk over its bins serves them all
                    const int32_t g = g_of[k];
                    const uint64_t* h = hist + (((size_t)p * gstride + g) << db);
                    uint64_t cum = 0, bin = 0;
                    int64_t last_bin = -1;
                    for (; k < nt && g_of[k] == g; ++k) {
                        while (bin < nb && cum + h[bin] <= r_of[k]) cum += h[bin++];
                        if (bin == nb)
                            return mhx_fail(MHX_EHIP, "%s: the histogram of a pass holds fewer draws than the rank asks for (tensor changed during the call?)", who);
                        if ((int64_t)bin != last_bin) { next_prefix[nng++] = (pf[g] << db) | bin; last_bin = (int64_t)bin; }
                        g_of[k] = nng - 1;
                        r_of[k] -= cum;
                    }
                }
                std::copy(next_prefix.begin(), next_prefix.begin() + nng, pf);
                ngroups[p] = nng;
            }
            remaining = shift;
        }
        // after the last digit the prefix is the key
        for (int32_t p = 0; p < nparams; ++p)
            for (int k = 0; k < nt; ++k)
                res[(size_t)p * T + b0 + k] = mhx_select_key_value(prefix[(size_t)p * gstride + grp[(size_t)p * gstride + k]], keybits);
    }
    for (int32_t p = 0; p < nparams; ++p)
        for (int32_t j = 0; j < nranks; ++j) {
            const size_t k = (size_t)(std::lower_bound(u.begin(), u.end(), (uint64_t)ranks[j]) - u.begin());
            out[(size_t)p * nranks + j] = res[(size_t)p * T + k];
        }
    return MHX_OK;
}
