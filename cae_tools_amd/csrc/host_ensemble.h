// host_ensemble.h - host only: the moments of the VAE's draws and their verification against the target, cae_ensemble_moments and
// cae_ensemble_verify, over kernels_stateless.h; both cut a plane by ensemble_chunk.  Included by stateless_host.h alone.
#pragma once

// 4-pixel groups per chunk, for both entry points: one wave per (case, chunk), about 4096 wave items where the call is
// large enough, chunks of 64 .. CM_GROUPS groups.  It depends on n_case and plane alone, so the same call is cut, and the
// verification folded, in the same order every time; a call with few cases (VaeEngine.ensemble brings max_batch / K) is
// cut finer and still covers the device.  The moments fold nothing: there a pixel's result does not depend on the cut.
static int64_t ensemble_chunk(int64_t n_case, int64_t plane) {
    const int64_t groups = (plane + 3) / 4;
    const int64_t chunk = (n_case * groups / 4096 + 63) / 64 * 64;
    return chunk < 64 ? 64 : (chunk > CM_GROUPS ? CM_GROUPS : chunk);
}

static int64_t ensemble_chunks(int64_t n_case, int64_t plane) {
    const int64_t chunk = ensemble_chunk(n_case, plane);
    return ((plane + 3) / 4 + chunk - 1) / chunk;
}

// ---- ensemble moments --------------------------------------------------------------------------

int64_t cae_ensemble_moments_workspace_bytes(int64_t n_case, int64_t plane) {
    if (n_case < 1 || plane < 1) return 0;
    return n_case * plane * (int64_t)(2 * sizeof(double) + sizeof(float));
}

int cae_ensemble_moments(const float* draws, int64_t case_stride, int64_t draw_stride, int64_t n_case, int64_t plane,
                         int k_call, int k_done, int k_total, double vmin, double range, double* mean, double* sd,
                         void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (!draws || !mean || n_case < 1 || plane < 1 || k_total < 2 || k_call < 1 || k_done < 0 || k_done + (int64_t)k_call > k_total)
        return fail(CAE_ERR_ARG, "cae_ensemble_moments: bad argument (k_total >= 2, 1 <= k_call, k_done + k_call <= k_total)");
    if ((n_case > 1 && case_stride < 0) || (k_call > 1 && draw_stride < 0))
        return fail(CAE_ERR_ARG, "cae_ensemble_moments: negative stride");
    // the planes of one call must not overlap: both layouts, [case][draw] and [draw][case], and anything looser
    const bool case_major = case_stride >= (int64_t)(k_call - 1) * draw_stride + plane && (k_call == 1 || draw_stride >= plane);
    const bool draw_major = draw_stride >= (n_case - 1) * case_stride + plane && (n_case == 1 || case_stride >= plane);
    if (!case_major && !draw_major) return fail(CAE_ERR_ARG, "cae_ensemble_moments: the strides make planes overlap");
    if (((uintptr_t)draws & 3) || ((uintptr_t)mean & 7) || ((uintptr_t)sd & 7))
        return fail(CAE_ERR_ARG, "cae_ensemble_moments: pointers must be aligned to their element size");
    const bool first = k_done == 0, last = k_done + k_call == k_total;
    const int64_t n = n_case * plane;
    EmArgs a;
    memset(&a, 0, sizeof a);
    if (!(first && last)) {
        const int64_t need = cae_ensemble_moments_workspace_bytes(n_case, plane);
        if (workspace_short(workspace, workspace_bytes, need))
            return fail(CAE_ERR_ARG, "cae_ensemble_moments: draws delivered over several calls need a workspace of %lld bytes "
                                     "(cae_ensemble_moments_workspace_bytes)", (long long)need);
        a.w1 = (double*)workspace;
        a.w2 = a.w1 + n;
        a.w0 = (float*)(a.w2 + n);
    }
    const int64_t chunk = ensemble_chunk(n_case, plane), nch = ensemble_chunks(n_case, plane);
    if (nch > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_ensemble_moments: plane too large");
    a.y = draws, a.case_stride = case_stride, a.draw_stride = draw_stride, a.plane = plane;
    a.kc = k_call, a.K = k_total, a.nch = (int)nch, a.chunk = (int)chunk, a.items = n_case * nch;
    a.vmin = vmin, a.range = range, a.mean = mean, a.sd = sd;
    const dim3 grid((unsigned)ceil_capped(a.items, CM_WAVES, 65536));
    hipStream_t s = (hipStream_t)hip_stream;
    if (first && last) hipLaunchKernelGGL((k_ensemble_moments<true, true>), grid, dim3(256), 0, s, a);
    else if (first) hipLaunchKernelGGL((k_ensemble_moments<true, false>), grid, dim3(256), 0, s, a);
    else if (last) hipLaunchKernelGGL((k_ensemble_moments<false, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_ensemble_moments<false, false>), grid, dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- ensemble verification ---------------------------------------------------------------------

constexpr int64_t EV_MAX_BLOCKS = 8192;

static int64_t verify_blocks(int64_t n_case, int64_t plane) {
    const int64_t items = n_case * ensemble_chunks(n_case, plane);
    return items < EV_MAX_BLOCKS ? items : EV_MAX_BLOCKS;
}

int64_t cae_ensemble_verify_workspace_bytes(int64_t n_case, int64_t plane, int k_total) {
    if (n_case < 1 || plane < 1 || k_total < 2 || k_total > 64) return 0;
    const int64_t nch = ensemble_chunks(n_case, plane);
    const int64_t part = nch > 1 ? n_case * nch * EV_SUMS * (int64_t)sizeof(double) : 0;
    return part + verify_blocks(n_case, plane) * (k_total + 2) * (int64_t)sizeof(int64_t);
}

int cae_ensemble_verify(const float* draws, int64_t case_stride, int64_t draw_stride, const void* actual, int actual_kind,
                        int64_t actual_stride, int64_t n_case, int64_t plane, int k_total, double vmin, double range,
                        double* case_sums, int64_t* rank_counts, void* workspace, int64_t workspace_bytes,
                        void* hip_stream) {
    const CaseOperand A{actual, actual_kind, actual_stride};
    if (n_case < 0 || plane < 0 || k_total < 2 || k_total > 64 || !known(A))
        return fail(CAE_ERR_ARG, "cae_ensemble_verify: bad argument (n_case >= 0, plane >= 0, 2 <= k_total <= 64, a CAE_ELEM_* kind)");
    if (case_stride < 0 || draw_stride < 0 || A.stride < 0) return fail(CAE_ERR_ARG, "cae_ensemble_verify: negative stride");
    if (!is_finite(vmin) || !is_finite(range) || range < 0.0)
        return fail(CAE_ERR_ARG, "cae_ensemble_verify: vmin must be finite, range finite and not negative");
    if (n_case == 0 || plane == 0) return CAE_OK;
    if (!draws || !A.p || !case_sums || !rank_counts) return fail(CAE_ERR_ARG, "cae_ensemble_verify: null pointer");
    // extents in 128 bits: no stride, however large, wraps a product; what the kernel indexes stays below 2^60 elements
    const __int128 draws_of_case = (__int128)(k_total - 1) * draw_stride + plane;
    const __int128 cases_of_draw = (__int128)(n_case - 1) * case_stride + plane;
    if (draws_of_case + (__int128)(n_case - 1) * case_stride > ((__int128)1 << 60) || reaches(A, n_case, plane))
        return fail(CAE_ERR_ARG, "cae_ensemble_verify: an operand reaches 2^60 elements from its pointer");
    const bool case_major = case_stride >= draws_of_case && draw_stride >= plane;
    const bool draw_major = draw_stride >= cases_of_draw && (n_case == 1 || case_stride >= plane);
    if (!case_major && !draw_major) return fail(CAE_ERR_ARG, "cae_ensemble_verify: the strides make planes overlap");
    if (shorter(A, plane)) return fail(CAE_ERR_ARG, "cae_ensemble_verify: the target's case stride is shorter than the plane");
    if (((uintptr_t)draws & 3) || misaligned(A) || ((uintptr_t)case_sums & 7) || ((uintptr_t)rank_counts & 7))
        return fail(CAE_ERR_ARG, "cae_ensemble_verify: pointers must be aligned to their element size");
    const int64_t nch = ensemble_chunks(n_case, plane);
    if (nch > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_ensemble_verify: plane too large");
    const int64_t need = cae_ensemble_verify_workspace_bytes(n_case, plane, k_total);
    if (workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_ensemble_verify", need);
    const int64_t blocks = verify_blocks(n_case, plane);
    const int64_t part = nch > 1 ? n_case * nch * EV_SUMS : 0;          // doubles before the rank partials
    EvArgs a;
    memset(&a, 0, sizeof a);
    a.y = draws, a.case_stride = case_stride, a.draw_stride = draw_stride;
    a.a = (const unsigned char*)A.p, a.a_stride = A.stride, a.plane = plane;
    a.K = k_total, a.nch = (int)nch, a.chunk = (int)ensemble_chunk(n_case, plane), a.items = n_case * nch;
    a.vmin = vmin, a.range = range;
    a.sums = nch > 1 ? (double*)workspace : case_sums;
    a.ranks = (long long*)((double*)workspace + part);
    hipStream_t s = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)blocks);
    const size_t lds = (size_t)k_total * EV_PIX * sizeof(float);        // at most 64 KiB
    with_kind(A.kind, [&](auto KA) { hipLaunchKernelGGL((k_ensemble_verify<decltype(KA)::value>), grid, dim3(64), lds, s, a); });
    HIP_TRY(hipGetLastError());
    const int n_bin = k_total + 2;
    const int64_t fb = nch > 1 ? ceil_capped(n_case * EV_SUMS, 256, 4096) : 0;
    hipLaunchKernelGGL(k_verify_fold, dim3((unsigned)(n_bin + fb)), dim3(256), 0, s, (const double*)workspace, (long long)n_case,
                       (int)nch, case_sums, (const long long*)a.ranks, (int)blocks, n_bin, (long long*)rank_counts);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
