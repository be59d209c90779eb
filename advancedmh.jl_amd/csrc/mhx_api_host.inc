// mhx_api_host.inc -- the boundary's RETURN path: samples back on the host, which is what the reference's `sample` hands
// its caller (bundle_samples: ext/AdvancedMHMCMCChainsExt.jl:12-39, src/AdvancedMH.jl:80-104 build host containers).
//
// mhx_run_sample_to_host == mhx_run_sample + mhx_run_get_samples, overlapped: the schedule is cut into slabs of K saved
// samples; launches write alternating device slabs while the previous slab drains through hipMemcpyAsync on a second
// stream into the caller's buffer (page-locked: from mhx_host_alloc, or registered for the duration of the call).
// A tensor that fits into HBM also stays there (the diagnostics work on it); one that does not is streamed through two
// alternating slabs, so N is bounded by host memory, not by HBM.  A thinned run returns at the kernel rate, a save-all run at
// the link rate (PCIe Gen5 x16: C2 fp64 13.4 GB per 250 draws).
// Included inside namespace MHX_NS by mhx_api.hip.


// ---- the accept-compacted form (include/mhx.h: mhx_compact_hdr; host side: mhx_host_expand.cpp) ---------------------------------
// Three small kernels per slab, all on the sampler stream, behind the launches that filled the slab:
//   k_compact_mask     one thread per (sample, chain): do the bits of the chain's column [dim+1] differ from the sample before?
//                      a wave's ballot is one mask word; its popcount goes into rank[]
//   k_compact_scan     ONE block: exclusive scan of rank[] over (sample, word) + the block's header
//   k_compact_scatter  the set chains write their column to row k of their sample's payload at their rank (coalesced reads,
//                      compacted writes)
// They read the slab twice (13.4 GB per 250 transitions at C2: ~6 ms of device time against ~60 ms of link time for the block).
#if MHX_REAL64
#define MHX_REAL_BITS(v) ((unsigned long long)__double_as_longlong(v))
#else
#define MHX_REAL_BITS(v) ((unsigned)__float_as_uint(v))
#endif

__global__ void __launch_bounds__(256)
k_compact_mask(const mhx_real* __restrict__ S, const mhx_real* __restrict__ prev0, const int n, const int d1, const int words,
               const int bps /* blocks per sample */, unsigned long long* __restrict__ mask, unsigned* __restrict__ rank)
{
    const int i = (int)(blockIdx.x / (unsigned)bps), bx = (int)(blockIdx.x % (unsigned)bps);
    const int c = bx * 256 + (int)threadIdx.x;
    bool ch = false;
    if (c < n) {
        const mhx_real* cur = S + (size_t)i * d1 * n + c;
        const mhx_real* pv = i ? cur - (size_t)d1 * n : (prev0 ? prev0 + c : nullptr);
        if (!pv) ch = true;                          // sample 0 of the call: nothing precedes it
        else
            for (int k = d1 - 1; k >= 0; --k) ch |= MHX_REAL_BITS(cur[(size_t)k * n]) != MHX_REAL_BITS(pv[(size_t)k * n]);
    }
    const unsigned long long b = __ballot(ch);
    const int w = bx * 4 + (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && w < words) {
        mask[(size_t)i * words + w] = b;
        rank[(size_t)i * words + w] = (unsigned)__popcll(b);
    }
}

__global__ void __launch_bounds__(1024)
k_compact_scan(unsigned* __restrict__ rank, const long L, mhx_compact_hdr* __restrict__ hdr, const mhx_compact_hdr proto)
{
    __shared__ unsigned long long part[1024];
    const int t = (int)threadIdx.x;
    const long per = (L + 1023) / 1024, a = (long)t * per, b = a + per < L ? a + per : L;
    unsigned long long s = 0;
    for (long i = a; i < b; ++i) s += rank[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned long long v = t >= off ? part[t - off] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = part[t] - s;
    for (long i = a; i < b; ++i) { const unsigned v = rank[i]; rank[i] = (unsigned)run; run += v; }
    if (t == 1023) {
        mhx_compact_hdr h = proto;
        h.total_changed = part[1023];
        h.block_bytes = h.payload_offset + h.total_changed * h.dim1 * h.elem_bytes;
        *hdr = h;
    }
}

__global__ void __launch_bounds__(256)
k_compact_scatter(const mhx_real* __restrict__ S, const int n, const int d1, const int cnt, const int words, const int bps,
                  const unsigned long long* __restrict__ mask, const unsigned* __restrict__ rank, const unsigned long long total,
                  mhx_real* __restrict__ payload)
{
    const int i = (int)(blockIdx.x / (unsigned)bps), bx = (int)(blockIdx.x % (unsigned)bps);
    const int c = bx * 256 + (int)threadIdx.x;
    if (c >= n) return;
    const int w = c >> 6;
    const unsigned long long bits = mask[(size_t)i * words + w];
    if (!((bits >> (c & 63)) & 1ull)) return;
    const unsigned long long first = rank[(size_t)i * words];
    const unsigned long long m = (i + 1 < cnt ? (unsigned long long)rank[(size_t)(i + 1) * words] : total) - first;
    const unsigned long long r = rank[(size_t)i * words + w] - first + (unsigned long long)__popcll(bits & ((1ull << (c & 63)) - 1ull));
    const mhx_real* col = S + (size_t)i * d1 * n + c;
    mhx_real* dst = payload + first * (unsigned long long)d1 + r;
    for (int k = 0; k < d1; ++k) dst[(size_t)k * m] = col[(size_t)k * n];
}

// A pageable destination the host threads are about to fill: ask for transparent huge pages on its 2 MiB-aligned interior
// (a hint: no effect where THP is off or the pages exist already).  A freshly allocated tensor -- what a `sample` call makes -- is
// then faulted in by the expanding threads 2 MiB at a time instead of 4 KiB (measured on the box: first fill 41 instead of 25 GB/s).
static void advise_huge_pages(void* p, size_t bytes)
{
    if (!p || bytes < ((size_t)8 << 20)) return;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost) return;     // page-locked already
    (void)hipGetLastError();
    const uintptr_t two = (uintptr_t)2 << 20, a = ((uintptr_t)p + two - 1) & ~(two - 1), e = ((uintptr_t)p + bytes) & ~(two - 1);
    if (e > a) (void)madvise((void*)a, e - a, MADV_HUGEPAGE);
}

static int compact_grow(void** p, size_t* cap, size_t need, bool host, int numa_node = -1)
{
    if (*cap >= need) return MHX_OK;
    if (*p) { if (host) (void)hipHostFree(*p); else (void)hipFree(*p); *p = nullptr; *cap = 0; }
    const size_t want = need + need / 4;             // a quarter of head room: blocks of a run differ by the luck of the draw
    // staging memory on the GPU's own memory node: its DMA engine writes there without crossing the socket link (measured on the
    // two-socket box: 53 against 30-37 GB/s for the blocks), and the expanding threads are kept to that node's CPUs
    if (host && numa_node >= 0) mhx_numa_prefer(numa_node);
    const hipError_t e = host ? hipHostMalloc(p, want, numa_node >= 0 ? hipHostMallocNumaUser : hipHostMallocDefault) : hipMalloc(p, want);
    if (host && numa_node >= 0) mhx_numa_default();
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return mhx_fail(MHX_ENOMEM, "mhx_run_sample_to_host: %zu bytes of %s staging: %s", want, host ? "page-locked host" : "device", hipGetErrorString(e)); }
    *cap = want;
    return MHX_OK;
}

// runs on an expander thread before a block is read: its copy has landed
static int compact_wait(void* arg)
{
    compact_pair* P = (compact_pair*)arg;
    (void)hipSetDevice(P->device);
    hipError_t e = hipEventSynchronize(P->c1);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, P->c0, P->c1);
    if (e != hipSuccess) return mhx_fail(MHX_EHIP, "mhx_run_sample_to_host: waiting for a block's copy: %s", hipGetErrorString(e));
    P->link_ms += ms;
    return MHX_OK;
}

static int compact_setup(mhx_ctx* ctx)
{
    for (compact_pair& P : ctx->cpair) {
        P.device = ctx->device;
        if (P.c0) continue;
        HIP_TRY(hipEventCreateWithFlags(&P.c0, hipEventBlockingSync));
        HIP_TRY(hipEventCreateWithFlags(&P.c1, hipEventBlockingSync));
        HIP_TRY(hipEventCreateWithFlags(&P.scattered, hipEventDisableTiming));
    }
    if (!ctx->hdr_pinned) HIP_TRY(hipHostMalloc((void**)&ctx->hdr_pinned, 3 * sizeof(mhx_compact_hdr), hipHostMallocDefault));
    const int want_t = opt_int(ctx, "HOST_THREADS", 0), want_c = opt_int(ctx, "HOST_CHUNK", 0);
    int want_n = -1;
    if (opt_int(ctx, "HOST_NUMA", 1) != 0) {                      // HOST_NUMA = 0: no placement (A/B)
        char bus[32] = {0};
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, ctx->device) == hipSuccess) want_n = mhx_numa_node_of_pci(bus);
        else (void)hipGetLastError();
    }
    if (ctx->expander && (ctx->expander_threads != want_t || ctx->expander_chunk != want_c || ctx->expander_numa != want_n)) {
        mhx_expander_destroy(ctx->expander);
        ctx->expander = nullptr;
        for (compact_pair& P : ctx->cpair)           // staging placed for the old setting
            if (P.host) { (void)hipHostFree(P.host); P.host = nullptr; P.host_cap = 0; }
    }
    if (!ctx->expander) {
        ctx->expander = mhx_expander_create(want_t, want_c, want_n);
        ctx->expander_threads = want_t;
        ctx->expander_chunk = want_c;
        ctx->expander_numa = want_n;
    }
    return MHX_OK;
}

static int host_streams(mhx_ctx* ctx)
{
    if (ctx->copy_stream) return MHX_OK;
    HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&ctx->slab_done[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->slab_free[i], hipEventDisableTiming));
    }
    return MHX_OK;
}

// page-lock [p, p + bytes) unless it already is (mhx_host_alloc / hipHostMalloc / registered by the caller);
// *mine says whether this call registered it.  Failure to register is not an error: the copy then runs pageable.
static void host_pin(mhx_ctx* ctx, void* p, size_t bytes, bool* mine)
{
    *mine = false;
    if (!p || !bytes) return;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost) return;
    (void)hipGetLastError();
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) { *mine = true; ++ctx->pins_registered; }
    else (void)hipGetLastError();
}

struct host_pin_guard {
    mhx_ctx* ctx;
    void* p[2] = {nullptr, nullptr};
    explicit host_pin_guard(mhx_ctx* c) : ctx(c) {}
    ~host_pin_guard()
    {
        for (void* q : p)
            if (q && hipHostUnregister(q) == hipSuccess) ++ctx->pins_released;
    }
};

// Every exit of the slab loop -- the normal one and every error return -- first waits for BOTH streams: a D2H copy still in
// flight targets the caller's buffer, which the pin guard is about to unregister and the caller may free.  Declared after the
// pin guard and the view guard, so it unwinds before them.  An exit that did not complete also leaves the run without a
// half-described tensor (n_saved / rec_n / the statistics view are reset).
struct stream_drain_guard {
    mhx_ctx* ctx; mhx_run* r; bool completed = false;
    stream_drain_guard(mhx_ctx* c, mhx_run* run) : ctx(c), r(run) {}
    ~stream_drain_guard()
    {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
        if (ctx->expander) (void)mhx_expander_drain(ctx->expander);       // no host thread still writes the caller's tensor
        if (!completed) { r->n_saved = 0; r->rec_n = 0; r->watch_count = 0; r->rec_loga_view = nullptr; (void)hipGetLastError(); }
    }
};

struct sample_view_guard {                   // the run's sample buffer pointers, restored on every exit path
    mhx_run* r; mhx_real* s; unsigned char* a;
    explicit sample_view_guard(mhx_run* run) : r(run), s(run->d_samples), a(run->d_accepted) {}
    ~sample_view_guard() { r->d_samples = s; r->d_accepted = a; }
};

int api_run_sample_to_host(mhx_run* r, const mhx_schedule* s, mhx_real* host_samples, uint8_t* host_accepted, int slab_samples)
{
    if (!r || !s) return mhx_fail(MHX_EINVAL, "mhx_run_sample_to_host: NULL argument");
    if (!r->initialised) return mhx_fail(MHX_ESTATE, "mhx_run_sample_to_host: call mhx_run_init first");
    if (r->tmp_R)
        return mhx_fail(MHX_ESTATE, "mhx_run_sample_to_host: a tempered run is not streamed to the host -- the accept-compacted return path takes a "
                                    "rejected transition for a repeat of the row above, and a swap breaks that: mhx_run_sample, then mhx_run_rung");
    if (r->adp)
        return mhx_fail(MHX_ESTATE, "mhx_run_sample_to_host: an adaptive run is not streamed to the host (the accept-compacted return path is left "
                                    "out): mhx_run_sample, then mhx_run_get_samples");
    if (!host_samples) return mhx_fail(MHX_EINVAL, "mhx_run_sample_to_host: samples is NULL (use mhx_run_sample to keep nothing)");
    if (s->n_samples < 1 || s->thinning < 1 || s->discard_initial < 0 || s->num_warmup < 0)
        return mhx_fail(MHX_EINVAL, "mhx_run_sample_to_host: bad schedule (N=%d discard=%d thinning=%d warmup=%d slab=%d)",
                        s->n_samples, s->discard_initial, s->thinning, s->num_warmup, slab_samples);
    if (slab_samples == INT32_MIN) return mhx_fail(MHX_EINVAL, "mhx_run_sample_to_host: slab_samples = INT32_MIN has no magnitude");
    mhx_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    uint64_t nT = 0, nA = 0;
    schedule_counts(s, &nT, &nA);
    if (r->tau + nT >= 0xffffffffull) return mhx_fail(MHX_EINVAL, "step counter would exceed 2^32-1; start a new seed");
    int rc = host_streams(ctx);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t N = (size_t)s->n_samples, n = (size_t)r->n, d1 = (size_t)r->dim + 1;
    const size_t rec = d1 * n * sizeof(mhx_real);            // one saved sample: [dim+1][nchains]
    // slab size: 256 MiB unless told otherwise -- long enough to run the link at its rate, short enough that the tail (the
    // last slab's copy, which nothing overlaps) stays small; at least one sample, at most the schedule
    size_t K = slab_samples ? (size_t)std::abs(slab_samples) : std::max<size_t>(1, ((size_t)256 << 20) / rec);
    K = std::min(K, N);
    // the accept-compacted form (include/mhx.h): context option HOST_COMPACT = 1 / 0, else when rows repeat (thinning == 1) and there
    // are chains enough for the host threads to share
    const bool compact = opt_int(ctx, "HOST_COMPACT", s->thinning == 1 && r->n >= 1024) != 0;
    if (compact) {
        K = std::min<size_t>(K, (size_t)0xffffffffull / n);                     // a block's ranks are 32-bit
        rc = compact_setup(ctx);
        if (rc) return rc;
        for (compact_pair& P : ctx->cpair) { P.used = false; P.link_ms = 0.0; }
        (void)mhx_expander_busy_seconds(ctx->expander, 1);
    }
    // Where the slabs live: when the whole tensor fits into HBM (what is allocated already, or 7/8 of what is free) the slabs
    // are consecutive pieces of it and the device keeps the tensor -- the diagnostics entry points work as after
    // mhx_run_sample; otherwise (or with slab_samples < 0) two slabs alternate and the device keeps nothing.
    bool ring = slab_samples < 0 && N > K;
    if (!ring && N > K && r->samples_cap < N * rec) {
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        if (N * (rec + n) > (fr + r->samples_cap) / 8 * 7) ring = true;
    }
    const size_t nslab = ring ? 2 : (N + K - 1) / K;
    const size_t dev_samples = ring ? 2 * K : N;
    rc = ensure_buffer((void**)&r->d_samples, &r->samples_cap, dev_samples * rec, "mhx_run_sample_to_host", "sample buffer");
    if (rc) return rc;
    rc = ensure_buffer((void**)&r->d_accepted, &r->accepted_cap, dev_samples * n, "mhx_run_sample_to_host", "accept-flag buffer");
    if (rc) return rc;
    host_pin_guard pins(ctx);
    bool mine = false;
    if (compact) advise_huge_pages(host_samples, N * rec);
    if (!compact) {                      // the compacted path writes the caller's buffers with the CPU: nothing to page-lock
        host_pin(ctx, host_samples, N * rec, &mine);
        if (mine) pins.p[0] = host_samples;
        host_pin(ctx, host_accepted, N * n, &mine);
        if (mine) pins.p[1] = host_accepted;
    }
    r->host_stats = mhx_host_stats{};
    r->host_stats.tensor_bytes = N * rec + (host_accepted ? N * n : 0);
    r->host_stats.compact = compact ? 1 : 0;
    r->host_stats.ring = ring ? 1 : 0;
    r->host_stats.threads = compact ? mhx_expander_threads(ctx->expander) : 0;

    r->stats = mhx_stats{};
    r->stats.kernel_variant = r->variant;
    r->stats.reduce_lanes = r->coop_L;
    r->stats.dtype = r->dtype;
    r->stats.normal_gen = r->normal_gen;
    r->stats.factor_band = r->kind == RUN_EMCEE ? r->emcee_band : -1;
    unsigned long long acc_before = 0, acc_after = 0;
    rc = run_total_accepts(r, &acc_before);
    if (rc) return rc;
    r->acc_total_known = false;          // (mhx_run_sample's copy of the counter: this call moves it)
    r->n_saved = 0;                      // the device buffer holds slabs, not the tensor: diagnostics need mhx_run_sample
    r->moments_mode = false;
    r->rec_n = 0;
    r->watch_count = 0;
    r->rec_loga_view = nullptr;
    if (r->kind == RUN_RAM) { rc = ram_prepare_step_stats(r, s, nA); if (rc) return rc; }

    sample_view_guard view(r);
    stream_drain_guard drain(ctx, r);    // from here on no path leaves with a copy in flight
#ifdef MHX_TOOLS_BUILD
    // test hook of the tools build: option FAULT_SLAB = k makes slab k (0-based) fail AFTER the copies of the earlier slabs were
    // enqueued -- the error path of a real hipError in the middle of a call (tests/test_gpu_host_path.py)
    const char* fault_env = opt(r->ctx, "FAULT_SLAB");
    const long fault_slab = fault_env ? atol(fault_env) : -1;
#endif
    mhx_real* const slab_s = view.s;
    unsigned char* const slab_a = view.a;
    const uint64_t tau0 = r->tau, di = (uint64_t)s->discard_initial, th = (uint64_t)s->thinning;
    uint64_t done_t = 0;                 // transitions of this call executed so far
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    for (size_t i0 = 0, c = 0; i0 < N; i0 += K, ++c) {
        const int b = (int)(c & 1);
#ifdef MHX_TOOLS_BUILD
        if ((long)c == fault_slab) return mhx_fail(MHX_EHIP, "mhx_run_sample_to_host: injected failure at slab %zu (option FAULT_SLAB)", c);
#endif
        const size_t cnt = std::min(K, N - i0);
        const size_t at = ring ? (size_t)b * K : i0;                                   // first sample slot of this slab on the device
        if (ring && c >= 2 && !compact) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->slab_free[b], 0));   // its previous contents have left (compacted: they left through kernels of this stream)
        r->d_samples = slab_s + at * d1 * n;
        r->d_accepted = slab_a + at * n;
        if (r->kind == RUN_RAM) r->rec_loga_view = r->d_rec_loga + i0 * n;     // the statistics stay whole on the device: [N][n]
        int slot = 0;
        if (i0 == 0 && di == 0) {
            // sample 1 is the current state itself (test/runtests.jl:203-213: chain[1].params == initial_params)
            if (r->kind == RUN_EMCEE) { int rcs = emcee_sync_state(r, 1); if (rcs) return rcs; }
            const unsigned grid = (unsigned)((r->n + 255) / 256);
            hipLaunchKernelGGL(k_record_state, dim3(grid), dim3(256), 0, ctx->stream, r->d_x, r->d_lp, r->d_last,
                               r->d_samples, r->d_accepted, r->n, (long)r->n, r->dim, 0L);
            HIP_TRY(hipGetLastError());
            slot = 1;
        }
        const uint64_t target_t = di + (uint64_t)(i0 + cnt - 1) * th;      // transition that produces the slab's last sample
        const uint64_t nsteps = target_t - done_t;
        const uint32_t save_next = (size_t)slot < cnt ? (uint32_t)(tau0 + di + (uint64_t)(i0 + (size_t)slot) * th) : MHX_NO_SAVE;
        if (nsteps) {
            const uint64_t adapt = done_t < nA ? std::min<uint64_t>(nA - done_t, nsteps) : 0;
            switch (r->kind) {
            case RUN_RWMH: rc = rwmh_advance(r, nsteps, save_next, slot, (int)th); break;
            case RUN_EMCEE: rc = emcee_advance(r, nsteps, save_next, slot, (int)th); break;
            case RUN_MALA: rc = mala_advance(r, nsteps, save_next, slot, (int)th); break;
            default: rc = ram_advance(r, nsteps, adapt, save_next, slot, (int)th); break;
            }
            if (rc) return rc;
        }
        done_t = target_t;
        ++r->host_stats.slabs;
        if (compact) {
            // ---- the slab leaves as ONE block: masks + ranks + accept flags + the changed columns
            compact_pair& P = ctx->cpair[c % 3];
            if (P.used) mhx_expander_wait(ctx->expander, P.seq);              // block c - 3 is expanded: the pair's buffers are free
            const uint32_t words = (uint32_t)((n + 63) / 64);
            const size_t nw = cnt * words, po = mhx_compact_payload_offset((uint32_t)cnt, words, (uint32_t)n);
            rc = compact_grow((void**)&P.dev_fixed, &P.dev_fixed_cap, po, false);
            if (rc) return rc;
            unsigned long long* const d_mask = (unsigned long long*)(P.dev_fixed + sizeof(mhx_compact_hdr));
            unsigned* const d_rank = (unsigned*)(P.dev_fixed + sizeof(mhx_compact_hdr) + 8 * nw);
            unsigned char* const d_acc = P.dev_fixed + sizeof(mhx_compact_hdr) + 8 * nw + ((4 * nw + 7) & ~(size_t)7);
            // the sample before the slab: the row above in the tensor, or (ring) the last row of the other slab, which the next
            // launches overwrite only after these kernels (same stream)
            const mhx_real* prev0 = c == 0 ? nullptr : (ring ? slab_s + ((size_t)(1 - b) * K + (K - 1)) * d1 * n : slab_s + (i0 - 1) * d1 * n);
            const int bps = (int)((n + 255) / 256);
            mhx_compact_hdr proto{};
            proto.magic = MHX_COMPACT_MAGIC; proto.elem_bytes = (uint32_t)sizeof(mhx_real); proto.dim1 = (uint32_t)d1; proto.nchains = (uint32_t)n;
            proto.first_sample = i0; proto.count = (uint32_t)cnt; proto.words = words; proto.payload_offset = po;
            hipLaunchKernelGGL(k_compact_mask, dim3((unsigned)(bps * cnt)), dim3(256), 0, ctx->stream, r->d_samples, prev0, (int)n, (int)d1, (int)words, bps, d_mask, d_rank);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, d_rank, (long)nw, (mhx_compact_hdr*)P.dev_fixed, proto);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(d_acc, r->d_accepted, cnt * n, hipMemcpyDeviceToDevice, ctx->stream));
            mhx_compact_hdr* const hh = ctx->hdr_pinned + (c % 3);
            HIP_TRY(hipMemcpyAsync(hh, P.dev_fixed, sizeof(mhx_compact_hdr), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));                          // the block's size is a result of the device
            const size_t pay = (size_t)hh->total_changed * d1 * sizeof(mhx_real);
            rc = compact_grow((void**)&P.dev_pay, &P.dev_pay_cap, pay, false);
            if (rc) return rc;
            rc = compact_grow((void**)&P.host, &P.host_cap, po + pay, true, ctx->expander_numa);
            if (rc) return rc;
            if (pay) {
                hipLaunchKernelGGL(k_compact_scatter, dim3((unsigned)(bps * cnt)), dim3(256), 0, ctx->stream, r->d_samples, (int)n, (int)d1, (int)cnt, (int)words, bps,
                                   d_mask, d_rank, (unsigned long long)hh->total_changed, (mhx_real*)P.dev_pay);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(P.scattered, ctx->stream));
            HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, P.scattered, 0));
            HIP_TRY(hipEventRecord(P.c0, ctx->copy_stream));
            HIP_TRY(hipMemcpyAsync(P.host, P.dev_fixed, po, hipMemcpyDeviceToHost, ctx->copy_stream));
            if (pay) HIP_TRY(hipMemcpyAsync(P.host + po, P.dev_pay, pay, hipMemcpyDeviceToHost, ctx->copy_stream));
            HIP_TRY(hipEventRecord(P.c1, ctx->copy_stream));
            mhx_expand_job job;
            job.block = P.host; job.samples = host_samples; job.accepted = host_accepted; job.n_samples = (int64_t)N;
            job.wait = compact_wait; job.wait_arg = &P;
            P.seq = mhx_expander_submit(ctx->expander, job);
            P.used = true;
            r->host_stats.wire_bytes += po + pay;
            continue;
        }
        r->host_stats.wire_bytes += cnt * rec + (host_accepted ? cnt * n : 0);
        HIP_TRY(hipEventRecord(ctx->slab_done[b], ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, ctx->slab_done[b], 0));
        HIP_TRY(hipMemcpyAsync((char*)host_samples + i0 * rec, r->d_samples, cnt * rec, hipMemcpyDeviceToHost, ctx->copy_stream));
        if (host_accepted)
            HIP_TRY(hipMemcpyAsync(host_accepted + i0 * n, r->d_accepted, cnt * n, hipMemcpyDeviceToHost, ctx->copy_stream));
        HIP_TRY(hipEventRecord(ctx->slab_free[b], ctx->copy_stream));
    }
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
    if (compact) {
        rc = mhx_expander_drain(ctx->expander);                                  // the caller's tensor is whole
        if (rc) return rc;
        for (const compact_pair& P : ctx->cpair) r->host_stats.link_ms += P.link_ms;
        r->host_stats.expand_ms = 1e3 * mhx_expander_busy_seconds(ctx->expander, 1);
    }
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    rc = run_total_accepts(r, &acc_after);
    if (rc) return rc;
    r->acc_total_host = acc_after;
    r->acc_total_known = r->kind != RUN_EMCEE;
    r->stats.kernel_ms = ms;             // the sampler kernels INCLUDING their waits for a free slab
    r->stats.transitions = nT * (uint64_t)r->n;
    r->stats.accepted = acc_after - acc_before;
    r->stats.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    (void)nslab;
    if (!ring) r->n_saved = s->n_samples;            // the device holds the whole tensor too
    drain.completed = true;
    return MHX_OK;
}
