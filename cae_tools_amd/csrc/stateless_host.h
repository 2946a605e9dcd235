// stateless_host.h - host only: the entry points of cae_hip.h that use no engine (loader, evaluator, ensemble moments and verification, case
// pages, per-pixel skill sums, power spectra, structural similarity, interpolation baseline, scene apply, value distributions, skill by stratum, neighbourhood skill, permutation importance, prediction intervals, novelty) over
// kernels_stateless.h, kernels_spectra.h, kernels_ssim.h, kernels_baseline.h, kernels_hist.h, kernels_strata.h, kernels_fss.h, kernels_importance.h, kernels_quantile.h, kernels_neighbours.h and kernels_scene.h.  Included by engine.hip alone, at the place
// this code has always had in it.
#pragma once
#include <type_traits>

// ---- the vocabulary of the entry points below: element kinds, case operands, grid sizes ---------------

static int elem_bytes(int kind) { return kind == CAE_ELEM_F32 || kind == CAE_ELEM_F32_BE ? 4 : 8; }
static bool kind_known(int kind) { return kind >= CAE_ELEM_F32 && kind <= CAE_ELEM_F64_BE; }

// One operand of a case kernel: channel 0 of the cases, `stride` elements from one case to the next.  The checks are
// functions over it; each entry point calls the ones it has always called, in its own order and under its own texts.
struct CaseOperand {
    const void* p;
    int kind;
    int64_t stride;
};
static bool known(const CaseOperand& o) { return kind_known(o.kind); }
static bool shorter(const CaseOperand& o, int64_t plane) { return o.stride < plane; }
static bool misaligned(const CaseOperand& o) { return (uintptr_t)o.p % elem_bytes(o.kind) != 0; }
// the last case ends above 2^60 elements from the pointer; in 128 bits, so that no stride, however large, wraps the product
static bool reaches(const CaseOperand& o, int64_t n_case, int64_t plane) {
    return (__int128)(n_case - 1) * o.stride + plane > ((__int128)1 << 60);
}
// no workspace of `need` bytes, 8 bytes aligned
static bool workspace_short(const void* ws, int64_t bytes, int64_t need) { return !ws || bytes < need || ((uintptr_t)ws & 7); }

// ceil(n / per), at most cap: so many workgroups for n items (the grid-stride kernels walk the rest)
static int64_t ceil_capped(int64_t n, int64_t per, int64_t cap) {
    const int64_t b = (n + per - 1) / per;
    return b < cap ? b : cap;
}

// The kind dispatch: f(std::integral_constant<int, K>()) for the run-time element kind, which the caller has checked
// (kind_known).  The kind-templated kernels are instantiated through it alone, the kinds in ascending order and "none"
// last, as the switches it replaces had them: a kernel's place in the code object follows the order of instantiation,
// and moving code inside the code object has cost the training step time before.
template <class F>
static void with_kind(int kind, F&& f) {
    switch (kind) {
    case CAE_ELEM_F32: f(std::integral_constant<int, 0>()); break;
    case CAE_ELEM_F32_BE: f(std::integral_constant<int, 1>()); break;
    case CAE_ELEM_F64: f(std::integral_constant<int, 2>()); break;
    default: f(std::integral_constant<int, 3>()); break;
    }
}

// the same for an optional operand: kind -1 stands for "none"
template <class F>
static void with_kind_or_none(int kind, F&& f) {
    switch (kind) {
    case CAE_ELEM_F32: f(std::integral_constant<int, 0>()); break;
    case CAE_ELEM_F32_BE: f(std::integral_constant<int, 1>()); break;
    case CAE_ELEM_F64: f(std::integral_constant<int, 2>()); break;
    case CAE_ELEM_F64_BE: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, -1>()); break;
    }
}

extern "C" {

// ---- loader -------------------------------------------------------------------------------------

int cae_scan_f32(const float* x, int64_t n, void* hip_stream, double* out3) {
    if (!x || n < 1 || !out3) return fail(CAE_ERR_ARG, "cae_scan_f32: bad argument");
    hipStream_t s = (hipStream_t)hip_stream;
    const int blocks = (int)ceil_capped(n, 256 * 16, 1024);
    double* part = nullptr;
    HIP_TRY(hipMalloc(&part, (size_t)blocks * 3 * sizeof(double)));
    hipLaunchKernelGGL(k_scan, dim3(blocks), dim3(256), 0, s, x, (long long)n, part);
    std::vector<double> host((size_t)blocks * 3);
    hipError_t ce = hipMemcpyAsync(host.data(), part, host.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (ce == hipSuccess) ce = hipStreamSynchronize(s);
    (void)hipFree(part);
    if (ce != hipSuccess) return fail(CAE_ERR_HIP, "cae_scan_f32: %s", hipGetErrorString(ce));
    double cnt = 0, lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < blocks; i++) {
        cnt += host[3 * i];
        lo = std::fmin(lo, host[3 * i + 1]);
        hi = std::fmax(hi, host[3 * i + 2]);
    }
    out3[0] = cnt;
    out3[1] = lo;
    out3[2] = hi;
    return CAE_OK;
}

int cae_normalise_pack_rows(const float* src, int64_t n, int c_src, int64_t hw, float* dst, int c_dst, int c_off,
                            float vmin, float range, int enable, const int32_t* dst_row_dev, void* hip_stream) {
    if (!src || !dst || n < 1 || c_src < 1 || hw < 1 || c_off < 0 || c_off + c_src > c_dst)
        return fail(CAE_ERR_ARG, "cae_normalise_pack: bad argument");
    if (n > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_normalise_pack: more than 2^31 - 1 rows");
    const long long total = (long long)n * c_src * hw;
    const int blocks = (int)ceil_capped(total, 256 * 8, 8192);
    hipLaunchKernelGGL(k_normalise_pack, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, src, total, c_src,
                       (long long)hw, dst, c_dst, c_off, vmin, range, enable, (const int*)dst_row_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_normalise_pack(const float* src, int64_t n, int c_src, int64_t hw, float* dst, int c_dst, int c_off,
                       float vmin, float range, int enable, void* hip_stream) {
    return cae_normalise_pack_rows(src, n, c_src, hw, dst, c_dst, c_off, vmin, range, enable, nullptr, hip_stream);
}

int cae_invert_permutation(const int32_t* perm_dev, int64_t n, int32_t* inverse_dev, void* hip_stream) {
    if (!perm_dev || !inverse_dev || n < 1 || n > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_invert_permutation: bad argument");
    hipLaunchKernelGGL(k_invert_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const int*)perm_dev, (long long)n, (int*)inverse_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_denormalise_f64(const float* y, int64_t n, double vmin, double range, double* out, void* hip_stream) {
    if (!y || !out || n < 1) return fail(CAE_ERR_ARG, "cae_denormalise_f64: bad argument");
    const int blocks = (int)ceil_capped(n, 256 * 8, 8192);
    hipLaunchKernelGGL(k_denorm_f64, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, y, (long long)n, vmin, range, out);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_metric_sums(const float* y, const float* actual, const float* mask, int64_t n_inst, int64_t inst_elems,
                    double vmin, double range, double* sums, void* hip_stream) {
    if (!y || !actual || !sums || n_inst < 1 || inst_elems < 1 || n_inst > 65535)
        return fail(CAE_ERR_ARG, "cae_metric_sums: bad argument");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(sums, 0, (size_t)n_inst * 8 * sizeof(double), s));
    const int chunks = (int)ceil_capped(inst_elems, 256 * 16, 64);
    hipLaunchKernelGGL(k_metric_sums, dim3(chunks, (unsigned)n_inst), dim3(256), 0, s, y, actual, mask,
                       (long long)inst_elems, vmin, range, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_bswap32(void* x, int64_t n, void* hip_stream) {
    if (!x || n < 0 || ((uintptr_t)x & 15)) return fail(CAE_ERR_ARG, "cae_bswap32: bad argument (16-byte aligned device pointer)");
    if (n == 0) return CAE_OK;
    int blocks = (int)((n / 4 + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_bswap32, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, (unsigned*)x, (long long)n);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- evaluator -------------------------------------------------------------------------------

static int64_t case_chunks(int64_t plane) { return (plane + 4 * CM_GROUPS - 1) / (4 * CM_GROUPS); }

int64_t cae_case_measures_workspace_bytes(int64_t n_case, int64_t plane) {
    if (n_case < 1 || plane < 1) return 0;
    const int64_t nch = case_chunks(plane);
    return nch > 1 ? n_case * nch * 2 * (int64_t)sizeof(double) : 0;
}

int cae_case_measures(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                      int64_t actual_stride, int64_t n_case, int64_t plane, double* out, void* workspace,
                      int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!P.p || !A.p || !out || n_case < 1 || plane < 1 || !known(P) || !known(A))
        return fail(CAE_ERR_ARG, "cae_case_measures: bad argument");
    if (shorter(P, plane) || shorter(A, plane))
        return fail(CAE_ERR_ARG, "cae_case_measures: a case stride is shorter than the plane");
    if (misaligned(P) || misaligned(A) || ((uintptr_t)out & 7))
        return fail(CAE_ERR_ARG, "cae_case_measures: pointers must be aligned to their element size");
    const int64_t nch = case_chunks(plane);
    if (nch > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_case_measures: plane too large");
    const int64_t need = cae_case_measures_workspace_bytes(n_case, plane);
    if (need > 0 && workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_case_measures: needs a workspace of %lld bytes (cae_case_measures_workspace_bytes)",
                    (long long)need);
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t items = n_case * nch;
    double* dst = nch > 1 ? (double*)workspace : out;
    const dim3 grid((unsigned)ceil_capped(items, CM_WAVES, 8192));
    with_kind(P.kind, [&](auto KP) {
        with_kind(A.kind, [&](auto KA) {
            hipLaunchKernelGGL((k_case_measures<decltype(KP)::value, decltype(KA)::value>), grid, dim3(256), 0, s,
                               (const unsigned char*)P.p, (long long)P.stride, (const unsigned char*)A.p, (long long)A.stride,
                               (long long)plane, (int)nch, (long long)items, dst);
        });
    });
    HIP_TRY(hipGetLastError());
    if (nch > 1) {
        hipLaunchKernelGGL(k_case_fold, dim3((unsigned)ceil_capped(n_case, 256, 4096)), dim3(256), 0, s,
                           (const double*)workspace, (long long)n_case, (int)nch, out);
        HIP_TRY(hipGetLastError());
    }
    return CAE_OK;
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
    // one wave per (case, chunk of 4-pixel groups): about 4096 waves in all where the call is large enough, chunks of 64 ..
    // CM_GROUPS groups (nothing is folded, so the cut is free: a pixel's result does not depend on it)
    const int64_t groups = (plane + 3) / 4;
    int64_t chunk = (n_case * groups / 4096 + 63) / 64 * 64;
    chunk = chunk < 64 ? 64 : (chunk > CM_GROUPS ? CM_GROUPS : chunk);
    const int64_t nch = (groups + chunk - 1) / chunk;
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

// 4-pixel groups per chunk: cae_ensemble_moments' rule - about 4096 wave items where the call is large enough, chunks of
// 64 .. CM_GROUPS groups.  It depends on n_case and plane alone, so the same call folds in the same order every time; a
// call with few cases (VaeEngine.ensemble brings max_batch / K) is cut finer and still covers the device.
static int64_t verify_chunk(int64_t n_case, int64_t plane) {
    const int64_t groups = (plane + 3) / 4;
    const int64_t chunk = (n_case * groups / 4096 + 63) / 64 * 64;
    return chunk < 64 ? 64 : (chunk > CM_GROUPS ? CM_GROUPS : chunk);
}

static int64_t verify_chunks(int64_t n_case, int64_t plane) {
    const int64_t chunk = verify_chunk(n_case, plane);
    return ((plane + 3) / 4 + chunk - 1) / chunk;
}

static int64_t verify_blocks(int64_t n_case, int64_t plane) {
    const int64_t items = n_case * verify_chunks(n_case, plane);
    return items < EV_MAX_BLOCKS ? items : EV_MAX_BLOCKS;
}

int64_t cae_ensemble_verify_workspace_bytes(int64_t n_case, int64_t plane, int k_total) {
    if (n_case < 1 || plane < 1 || k_total < 2 || k_total > 64) return 0;
    const int64_t nch = verify_chunks(n_case, plane);
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
    if (!(vmin - vmin == 0.0) || !(range - range == 0.0) || range < 0.0)
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
    const int64_t nch = verify_chunks(n_case, plane);
    if (nch > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_ensemble_verify: plane too large");
    const int64_t need = cae_ensemble_verify_workspace_bytes(n_case, plane, k_total);
    if (workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_ensemble_verify: needs a workspace of %lld bytes (cae_ensemble_verify_workspace_bytes)",
                    (long long)need);
    const int64_t blocks = verify_blocks(n_case, plane);
    const int64_t part = nch > 1 ? n_case * nch * EV_SUMS : 0;          // doubles before the rank partials
    EvArgs a;
    memset(&a, 0, sizeof a);
    a.y = draws, a.case_stride = case_stride, a.draw_stride = draw_stride;
    a.a = (const unsigned char*)A.p, a.a_stride = A.stride, a.plane = plane;
    a.K = k_total, a.nch = (int)nch, a.chunk = (int)verify_chunk(n_case, plane), a.items = n_case * nch;
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

// ---- case pages ------------------------------------------------------------------------------

static int64_t range_blocks(int64_t n_case, int64_t plane) { return ceil_capped(n_case * case_chunks(plane), CM_WAVES, 8192); }

int64_t cae_case_range_workspace_bytes(int64_t n_case, int64_t plane) {
    if (n_case < 1 || plane < 1) return 0;
    return range_blocks(n_case, plane) * 3 * (int64_t)sizeof(double);
}

// The shared argument checks of cae_case_range / cae_render_cases: the source S and the optional operand B subtracted from
// it (a null pointer: none, and its kind and stride are not looked at).  The three texts of cae_case_measures; neither
// entry point has the 2^60 check.
static int case_pair_check(const char* who, const CaseOperand& S, const CaseOperand& B, int64_t plane) {
    if (!S.p || !known(S) || (B.p && !known(B))) return fail(CAE_ERR_ARG, "%s: bad argument", who);
    if (shorter(S, plane) || (B.p && shorter(B, plane)))
        return fail(CAE_ERR_ARG, "%s: a case stride is shorter than the plane", who);
    if (misaligned(S) || (B.p && misaligned(B)))
        return fail(CAE_ERR_ARG, "%s: pointers must be aligned to their element size", who);
    return CAE_OK;
}

int cae_case_range(const void* src, int src_kind, int64_t src_stride, const void* sub, int sub_kind, int64_t sub_stride,
                   int64_t n_case, int64_t plane, double* out, void* workspace, int64_t workspace_bytes,
                   void* hip_stream) {
    if (!out || ((uintptr_t)out & 7) || n_case < 1 || plane < 1) return fail(CAE_ERR_ARG, "cae_case_range: bad argument");
    const CaseOperand S{src, src_kind, src_stride}, B{sub, sub_kind, sub_stride};
    const int rc = case_pair_check("cae_case_range", S, B, plane);
    if (rc != CAE_OK) return rc;
    const int64_t nch = case_chunks(plane);
    if (nch > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_case_range: plane too large");
    const int64_t need = cae_case_range_workspace_bytes(n_case, plane);
    if (workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_case_range: needs a workspace of %lld bytes (cae_case_range_workspace_bytes)",
                    (long long)need);
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t blocks = range_blocks(n_case, plane);
    const dim3 grid((unsigned)blocks);
    with_kind(S.kind, [&](auto KS) {
        with_kind_or_none(B.p ? B.kind : -1, [&](auto KB) {
            hipLaunchKernelGGL((k_case_range<decltype(KS)::value, decltype(KB)::value>), grid, dim3(256), 0, s,
                               (const unsigned char*)S.p, (long long)S.stride, (const unsigned char*)B.p, (long long)B.stride,
                               (long long)plane, (int)nch, (long long)(n_case * nch), (double*)workspace);
        });
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_range_fold, dim3(1), dim3(256), 0, s, (const double*)workspace, (int)blocks, out);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_render_cases(const void* src, int src_kind, int64_t src_stride, const void* sub, int sub_kind, int64_t sub_stride,
                     const int32_t* cases, int64_t n_sel, int64_t n_case, int64_t height, int64_t width, double lo,
                     double hi, int flip_y, uint8_t* out, void* hip_stream) {
    if (!out || n_sel < 1 || n_case < 1 || height < 1 || width < 1 || ((uintptr_t)cases & 3))
        return fail(CAE_ERR_ARG, "cae_render_cases: bad argument");
    if (height * (width + 1) > 0x7fffffffLL || width > 0x7ffffffeLL)
        return fail(CAE_ERR_ARG, "cae_render_cases: image too large (height * (width + 1) must stay below 2^31)");
    if (!(lo - lo == 0.0) || !(hi - hi == 0.0) || !((hi - lo) - (hi - lo) == 0.0))
        return fail(CAE_ERR_ARG, "cae_render_cases: lo, hi and hi - lo must be finite");
    const CaseOperand S{src, src_kind, src_stride}, B{sub, sub_kind, sub_stride};
    const int rc = case_pair_check("cae_render_cases", S, B, height * width);
    if (rc != CAE_OK) return rc;
    const int64_t len = height * (width + 1);
    const int64_t nch = (len / 4 + RC_DWORDS - 1) / RC_DWORDS > 0 ? (len / 4 + RC_DWORDS - 1) / RC_DWORDS : 1;
    const int64_t items = n_sel * nch;
    const dim3 grid((unsigned)ceil_capped(items, CM_WAVES, 8192));
    with_kind(S.kind, [&](auto KS) {
        with_kind_or_none(B.p ? B.kind : -1, [&](auto KB) {
            hipLaunchKernelGGL((k_render_cases<decltype(KS)::value, decltype(KB)::value>), grid, dim3(256), 0,
                               (hipStream_t)hip_stream, (const unsigned char*)S.p, (long long)S.stride, (const unsigned char*)B.p,
                               (long long)B.stride, (const int*)cases, (long long)n_case, (unsigned)height, (unsigned)width, lo, hi,
                               flip_y, (int)nch, (long long)items, out);
        });
    });
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- per-pixel skill sums --------------------------------------------------------------------

static int64_t pixel_tiles(int64_t plane) {
    const int64_t t = (plane / 4 + PS_TILE - 1) / PS_TILE;      // (a head before the first 16-byte phase never adds a tile)
    return t > 0 ? t : 1;
}

// Cases per chunk.  The library's choice (case_chunk 0) is the longest chunk that still gives about PS_WAVE_ITEMS wave
// items - the waves the device holds at once, four on each of its 1024 SIMDs - and never fewer than PS_MIN_CHUNK cases:
// below that a chunk's partial (72 bytes per pixel, written and read again) outweighs what the chunk reads.  An item
// here costs bytes, unlike cae_case_measures' 16-byte partials: at 2000 cases of 256 x 256 the 32 000 items that call
// launches (chunks of 16 cases) took twice the time of 4096 (chunks of 125).
constexpr int64_t PS_WAVE_ITEMS = 4096;
constexpr int64_t PS_MIN_CHUNK = 8;

static int64_t pixel_chunk(int64_t n_case, int64_t plane, int64_t case_chunk) {
    if (case_chunk > 0) return case_chunk < n_case ? case_chunk : n_case;
    int64_t n_chunk = PS_WAVE_ITEMS / pixel_tiles(plane);
    if (n_chunk < 1) n_chunk = 1;
    int64_t chunk = (n_case + n_chunk - 1) / n_chunk;
    if (chunk < PS_MIN_CHUNK) chunk = PS_MIN_CHUNK;
    return chunk < n_case ? chunk : n_case;
}

int64_t cae_pixel_sums_workspace_bytes(int64_t n_case, int64_t plane, int64_t case_chunk) {
    if (n_case < 1 || plane < 1 || case_chunk < 0) return 0;
    const int64_t chunk = pixel_chunk(n_case, plane, case_chunk);
    const int64_t n_chunk = (n_case + chunk - 1) / chunk;
    return n_chunk > 1 ? n_chunk * PS_SUMS * plane * (int64_t)sizeof(double) : 0;
}

// cae_pixel_sums (shifts == NULL) and cae_pixel_sums_about (per-pixel shifts, `shift` unused)
static int pixel_sums_run(const CaseOperand& P, const CaseOperand& A, int64_t n_case, int64_t plane, double shift,
                          const double* shifts, int64_t case_chunk, double* sums, void* workspace, int64_t workspace_bytes,
                          void* hip_stream) {
    if (n_case < 0 || plane < 0 || case_chunk < 0 || !known(P) || !known(A) || !(shift - shift == 0.0))
        return fail(CAE_ERR_ARG, "cae_pixel_sums: bad argument");
    if (plane == 0) return CAE_OK;
    if (!sums || ((uintptr_t)sums & 7)) return fail(CAE_ERR_ARG, "cae_pixel_sums: sums_dev must be an 8-byte aligned pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    if (n_case == 0) {      // no case, no pair: nine planes of zeros
        HIP_TRY(hipMemsetAsync(sums, 0, (size_t)plane * PS_SUMS * sizeof(double), s));
        return CAE_OK;
    }
    if (!P.p || !A.p) return fail(CAE_ERR_ARG, "cae_pixel_sums: bad argument");
    if (shorter(P, plane) || shorter(A, plane))
        return fail(CAE_ERR_ARG, "cae_pixel_sums: a case stride is shorter than the plane");
    if (misaligned(P) || misaligned(A))
        return fail(CAE_ERR_ARG, "cae_pixel_sums: pointers must be aligned to their element size");
    const int ep = elem_bytes(P.kind), ea = elem_bytes(A.kind);
    const int64_t chunk = pixel_chunk(n_case, plane, case_chunk);
    const int64_t n_chunk = (n_case + chunk - 1) / chunk;
    const int64_t need = cae_pixel_sums_workspace_bytes(n_case, plane, case_chunk);
    if (need > 0 && workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_pixel_sums: needs a workspace of %lld bytes (cae_pixel_sums_workspace_bytes)",
                    (long long)need);
    PsArgs a;
    memset(&a, 0, sizeof a);
    // 16-byte loads: case 0 has an element where both operands are 16 bytes aligned, and every case stride keeps it
    int h = -1;
    for (int t = 3; t >= 0; t--)
        if ((((uintptr_t)P.p + (uintptr_t)t * ep) | ((uintptr_t)A.p + (uintptr_t)t * ea)) % 16 == 0) h = t;
    const bool keep = n_case == 1 || ((P.stride * ep) % 16 == 0 && (A.stride * ea) % 16 == 0);
    a.vec = h >= 0 && keep;
    a.head = a.vec ? (int)(h < plane ? h : plane) : 0;
    a.p = (const unsigned char*)P.p, a.a = (const unsigned char*)A.p;
    a.p_stride = P.stride, a.a_stride = A.stride, a.n_case = n_case, a.plane = plane;
    a.chunk = chunk, a.n_chunk = n_chunk;
    a.shift = shift, a.shifts = shifts;
    a.out = n_chunk > 1 ? (double*)workspace : sums;
    const int64_t n_tile = pixel_tiles(plane);
    if (n_tile > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_pixel_sums: plane too large");
    const dim3 grid((unsigned)n_tile, (unsigned)(n_chunk < 65535 ? n_chunk : 65535));     // one wave per workgroup
    with_kind(P.kind, [&](auto KP) {
        with_kind(A.kind, [&](auto KA) {
            constexpr int kp = decltype(KP)::value, ka = decltype(KA)::value;
            if (a.shifts) hipLaunchKernelGGL((k_pixel_sums<kp, ka, true>), grid, dim3(64), 0, s, a);
            else hipLaunchKernelGGL((k_pixel_sums<kp, ka, false>), grid, dim3(64), 0, s, a);
        });
    });
    HIP_TRY(hipGetLastError());
    if (n_chunk > 1) {
        const int64_t n = PS_SUMS * plane;
        hipLaunchKernelGGL(k_pixel_fold, dim3((unsigned)ceil_capped(n, 256, 8192)), dim3(256), 0, s, (const double*)workspace,
                           (long long)n_chunk, (long long)n, sums);
        HIP_TRY(hipGetLastError());
    }
    return CAE_OK;
}

int cae_pixel_sums(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                   int64_t actual_stride, int64_t n_case, int64_t plane, double shift, int64_t case_chunk, double* sums,
                   void* workspace, int64_t workspace_bytes, void* hip_stream) {
    return pixel_sums_run({pred, pred_kind, pred_stride}, {actual, actual_kind, actual_stride}, n_case, plane, shift, nullptr,
                          case_chunk, sums, workspace, workspace_bytes, hip_stream);
}

int cae_pixel_sums_about(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                         int64_t actual_stride, int64_t n_case, int64_t plane, const double* shifts, int64_t case_chunk,
                         double* sums, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (plane > 0 && n_case > 0 && (!shifts || ((uintptr_t)shifts & 7)))
        return fail(CAE_ERR_ARG, "cae_pixel_sums_about: shifts_dev must be an 8-byte aligned pointer");
    return pixel_sums_run({pred, pred_kind, pred_stride}, {actual, actual_kind, actual_stride}, n_case, plane, 0.0,
                          n_case > 0 ? shifts : nullptr, case_chunk, sums, workspace, workspace_bytes, hip_stream);
}

// ---- power spectra of prediction against target ---------------------------------------------------

// kx columns per band: what keeps the h x nb tile of three complex fields within 96 KiB of LDS, at most SP_MAX_NB and no
// more than the half plane has.  It depends on (h, w) alone, so a case is cut into the same bands in every call.
static int spectra_nb(int64_t h, int64_t w) {
    const int nbh = h <= SP_TILE_ELEMS / 4 ? 4 : (h <= SP_TILE_ELEMS / 2 ? 2 : 1);
    const int64_t wc = w / 2 + 1;
    const int nbw = wc >= 4 ? 4 : (wc >= 2 ? 2 : 1);
    return nbh < nbw ? nbh : nbw;
}

static int64_t spectra_bands(int64_t h, int64_t w) {
    const int nb = spectra_nb(h, w);
    return (w / 2 + 1 + nb - 1) / nb;
}

// the workspace in doubles: twiddles of h and of w (pairs), the cases' means and flags, the (case, band, bin) partials
static int64_t spectra_table_doubles(int64_t n_case, int64_t h, int64_t w) { return 2 * (h + w) + 4 * n_case; }

static bool spectra_sizes_ok(int64_t n_case, int64_t h, int64_t w, int64_t n_bin) {
    return n_case >= 0 && h >= 1 && h <= SP_MAX_SIDE && w >= 1 && w <= SP_MAX_SIDE && n_bin >= 1 &&
           n_bin <= ((int64_t)1 << 24) && n_case * spectra_bands(h, w) <= 0x7fffffffLL &&
           (__int128)n_case * spectra_bands(h, w) * n_bin < ((__int128)1 << 56);
}

int64_t cae_case_spectra_workspace_bytes(int64_t n_case, int64_t h, int64_t w, int64_t n_bin) {
    if (n_case < 1 || !spectra_sizes_ok(n_case, h, w, n_bin)) return 0;
    return (spectra_table_doubles(n_case, h, w) + n_case * spectra_bands(h, w) * n_bin * 4) * (int64_t)sizeof(double);
}

extern "C++" {

template <int NB>
static void launch_case_spectra(dim3 grid, size_t lds, hipStream_t s, const SpArgs& a) {
    static size_t granted = 64 * 1024;      // above it a kernel has to ask
    if (lds > granted) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_case_spectra<NB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        granted = lds;
    }
    hipLaunchKernelGGL((k_case_spectra<NB>), grid, dim3(SP_THREADS), lds, s, a);
}

}  // extern "C++"

int cae_case_spectra(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                     int64_t actual_stride, int64_t n_case, int64_t h, int64_t w, const double* wy, const double* wx,
                     const int32_t* bin, int64_t n_bin, double* sums, int32_t* counted, void* workspace,
                     int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!known(P) || !known(A) || !spectra_sizes_ok(n_case, h, w, n_bin))
        return fail(CAE_ERR_ARG, "cae_case_spectra: bad argument (CAE_ELEM_* kinds, n_case >= 0, 1 <= h, w <= %d, n_bin >= 1)", SP_MAX_SIDE);
    if (n_case == 0) return CAE_OK;
    const int64_t plane = h * w;
    if (!P.p || !A.p || !wy || !wx || !bin || !sums || !counted || !workspace)
        return fail(CAE_ERR_ARG, "cae_case_spectra: null pointer");
    if (shorter(P, plane) || shorter(A, plane))
        return fail(CAE_ERR_ARG, "cae_case_spectra: a case stride is shorter than the plane");
    if (reaches(P, n_case, plane) || reaches(A, n_case, plane))
        return fail(CAE_ERR_ARG, "cae_case_spectra: an operand reaches 2^60 elements from its pointer");
    if (misaligned(P) || misaligned(A) || ((uintptr_t)wy & 7) || ((uintptr_t)wx & 7) || ((uintptr_t)bin & 3) ||
        ((uintptr_t)sums & 7) || ((uintptr_t)counted & 3) || ((uintptr_t)workspace & 15))
        return fail(CAE_ERR_ARG, "cae_case_spectra: pointers must be aligned to their element size, the workspace to 16 bytes");
    const int64_t need = cae_case_spectra_workspace_bytes(n_case, h, w, n_bin);
    if (workspace_bytes < need)
        return fail(CAE_ERR_ARG, "cae_case_spectra: needs a workspace of %lld bytes (cae_case_spectra_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)hip_stream;
    const int nb = spectra_nb(h, w);
    const int64_t n_band = spectra_bands(h, w);
    double* ws = (double*)workspace;
    SpArgs a;
    memset(&a, 0, sizeof a);
    a.p = (const unsigned char*)pred, a.a = (const unsigned char*)actual;
    a.p_stride = pred_stride, a.a_stride = actual_stride, a.pk = pred_kind, a.ak = actual_kind;
    a.h = (int)h, a.w = (int)w, a.wc = (int)(w / 2 + 1), a.n_band = (int)n_band, a.n_bin = (int)n_bin;
    a.wy = wy, a.wx = wx, a.bin = (const int*)bin;
    double2* twh = (double2*)ws;
    double2* tww = twh + h;
    double* mu = ws + 2 * (h + w);
    a.twh = twh, a.tww = tww, a.mu = mu, a.part = ws + spectra_table_doubles(n_case, h, w);
    hipLaunchKernelGGL(k_spectra_twiddle, dim3((unsigned)(((h > w ? h : w) + 255) / 256)), dim3(256), 0, s, twh, (int)h, tww, (int)w);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_spectra_mean, dim3((unsigned)n_case), dim3(SP_THREADS), 0, s, a.p, pred_kind, (long long)pred_stride,
                       a.a, actual_kind, (long long)actual_stride, (long long)plane, mu, (int*)counted);
    HIP_TRY(hipGetLastError());
    const size_t tile = (size_t)h * nb * 3 * sizeof(double2), stage = (size_t)SP_THREADS * nb * (4 * sizeof(double) + sizeof(int));
    const size_t lds = h > SP_THREADS ? tile + stage : (tile > stage ? tile : stage);
    const dim3 grid((unsigned)(n_case * n_band));
    switch (nb) {
    case 4: launch_case_spectra<4>(grid, lds, s, a); break;
    case 2: launch_case_spectra<2>(grid, lds, s, a); break;
    default: launch_case_spectra<1>(grid, lds, s, a); break;
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_spectra_fold, dim3((unsigned)ceil_capped(n_case * n_bin * 4, 256, 8192)), dim3(256), 0, s,
                       (const double*)a.part, (long long)n_case, (int)n_band, (int)n_bin, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- structural similarity of prediction against target ---------------------------------------------

// the side of the next scale: 2 x 2 pooling with padding size mod 2 on both sides
static int64_t ssim_pooled(int64_t side) { return (side + 2 * (side & 1)) / 2; }

// the scales' shapes and the cut of each into (band, strip) items, from (h, w) alone; returns the items of one case
static int64_t ssim_plan(int64_t h, int64_t w, int n_scale, SsScale* sc, int64_t* plane_doubles) {
    int64_t per_case = 0, planes = 0;
    for (int s = 0; s < n_scale; s++) {
        sc[s].h = (int)h, sc[s].w = (int)w;
        sc[s].rb = ss_band_rows((int)h);
        const bool any = h >= SS_WIN && w >= SS_WIN;
        sc[s].n_band = any ? (int)((h - SS_HALO + sc[s].rb - 1) / sc[s].rb) : 0;
        sc[s].n_strip = any ? (int)((w - SS_HALO + SS_COLS - 1) / SS_COLS) : 0;
        per_case += (int64_t)sc[s].n_band * sc[s].n_strip;
        if (s > 0) planes += 2 * h * w;
        h = ssim_pooled(h), w = ssim_pooled(w);
    }
    if (plane_doubles) *plane_doubles = planes;
    return per_case;
}

static bool ssim_sizes_ok(int64_t n_case, int64_t h, int64_t w, int n_scale) {
    if (n_case < 0 || h < 1 || h > SS_MAX_SIDE || w < 1 || w > SS_MAX_SIDE || n_scale < 1 || n_scale > SS_SCALES) return false;
    SsScale sc[SS_SCALES];
    int64_t planes = 0;
    const int64_t per_case = ssim_plan(h, w, n_scale, sc, &planes);
    return (__int128)n_case * per_case <= 0x7fffffffLL && (__int128)n_case * planes < ((__int128)1 << 56);
}

int64_t cae_case_ssim_workspace_bytes(int64_t n_case, int64_t h, int64_t w, int n_scale) {
    if (n_case < 1 || !ssim_sizes_ok(n_case, h, w, n_scale)) return 0;
    SsScale sc[SS_SCALES];
    int64_t planes = 0;
    const int64_t per_case = ssim_plan(h, w, n_scale, sc, &planes);
    return n_case * (planes + 3 * per_case) * (int64_t)sizeof(double);
}

int cae_case_ssim(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                  int64_t actual_stride, int64_t n_case, int64_t h, int64_t w, int n_scale, double shift, double scale,
                  const double* window, double* sums, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!known(P) || !known(A) || !ssim_sizes_ok(n_case, h, w, n_scale))
        return fail(CAE_ERR_ARG, "cae_case_ssim: bad argument (CAE_ELEM_* kinds, n_case >= 0, 1 <= h, w <= %d, 1 <= n_scale <= %d)",
                    SS_MAX_SIDE, SS_SCALES);
    if (!(shift - shift == 0.0) || !(scale - scale == 0.0)) return fail(CAE_ERR_ARG, "cae_case_ssim: shift and scale must be finite");
    if (n_case == 0) return CAE_OK;
    const int64_t plane = h * w;
    if (!P.p || !A.p || !window || !sums) return fail(CAE_ERR_ARG, "cae_case_ssim: null pointer");
    if (shorter(P, plane) || shorter(A, plane))
        return fail(CAE_ERR_ARG, "cae_case_ssim: a case stride is shorter than the plane");
    if (reaches(P, n_case, plane) || reaches(A, n_case, plane))
        return fail(CAE_ERR_ARG, "cae_case_ssim: an operand reaches 2^60 elements from its pointer");
    if (misaligned(P) || misaligned(A) || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 7))
        return fail(CAE_ERR_ARG, "cae_case_ssim: pointers must be aligned to their element size, the workspace to 8 bytes");
    const int64_t need = cae_case_ssim_workspace_bytes(n_case, h, w, n_scale);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(CAE_ERR_ARG, "cae_case_ssim: needs a workspace of %lld bytes (cae_case_ssim_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)hip_stream;
    SsArgs a;
    memset(&a, 0, sizeof a);
    int64_t planes = 0;
    const int64_t per_case = ssim_plan(h, w, n_scale, a.s, &planes);
    a.n_scale = n_scale, a.n_case = n_case, a.items = n_case * per_case;
    a.shift = shift, a.scale = scale;
    for (int t = 0; t < SS_WIN; t++) a.win.g[t] = window[t];
    double* ws = (double*)workspace;
    a.part = ws + n_case * planes;
    a.s[0].x = (const unsigned char*)pred, a.s[0].y = (const unsigned char*)actual;
    a.s[0].x_stride = pred_stride, a.s[0].y_stride = actual_stride, a.s[0].xk = pred_kind, a.s[0].yk = actual_kind;
    int64_t first = 0;
    for (int k = 0; k < n_scale; k++) {
        SsScale& c = a.s[k];
        c.first = first;
        first += n_case * c.n_band * c.n_strip;
        if (k + 1 == n_scale) break;
        // the planes of scale k + 1: [case][x | y][h][w] doubles, pooled from scale k
        SsScale& d = a.s[k + 1];
        const int64_t per = (int64_t)d.h * d.w;
        d.x = (const unsigned char*)ws, d.y = (const unsigned char*)(ws + per);
        d.x_stride = d.y_stride = 2 * per, d.xk = d.yk = CAE_ELEM_F64;
        hipLaunchKernelGGL(k_ssim_pool, dim3((unsigned)ceil_capped(n_case * per, 256, 65536)), dim3(256), 0, s, c.x, c.xk,
                           (long long)c.x_stride, c.y, c.yk, (long long)c.y_stride, (long long)n_case, c.h, c.w,
                           k == 0 ? shift : 0.0, k == 0 ? scale : 1.0, ws);
        HIP_TRY(hipGetLastError());
        ws += n_case * 2 * per;
    }
    if (a.items > 0) {
        hipLaunchKernelGGL(k_case_ssim, dim3((unsigned)((a.items + 3) / 4)), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ssim_fold, dim3((unsigned)ceil_capped(n_case * n_scale * 3, 256, 4096)), dim3(256), 0, s, a, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- skill against interpolating the input ------------------------------------------------------------

// the (band, strip) items of one case, from (h_out, w_out) alone
static int64_t baseline_items(int64_t h_out, int64_t w_out) {
    return ((h_out + BL_ROWS - 1) / BL_ROWS) * ((w_out + BL_COLS - 1) / BL_COLS);
}

static bool baseline_sizes_ok(int64_t n_case, int64_t h_out, int64_t w_out) {
    return n_case >= 0 && h_out >= 1 && h_out <= BL_MAX_SIDE && w_out >= 1 && w_out <= BL_MAX_SIDE &&
           (__int128)n_case * baseline_items(h_out, w_out) <= 0x7fffffffLL;
}

int64_t cae_case_baseline_workspace_bytes(int64_t n_case, int64_t h_out, int64_t w_out) {
    if (n_case < 1 || !baseline_sizes_ok(n_case, h_out, w_out)) return 0;
    return n_case * baseline_items(h_out, w_out) * BL_SUMS * (int64_t)sizeof(double);
}

int cae_case_baseline(const void* low, int low_kind, int64_t low_stride, int64_t h_in, int64_t w_in, const void* pred,
                      int pred_kind, int64_t pred_stride, const void* actual, int actual_kind, int64_t actual_stride,
                      int64_t n_case, int64_t h_out, int64_t w_out, int mode, double* sums, double* field, void* workspace,
                      int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand L{low, low_kind, low_stride}, P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!known(L) || !known(A) || (P.p && !known(P)) || mode < CAE_INTERP_NEAREST ||
        mode > CAE_INTERP_BICUBIC || h_in < 1 || h_in > BL_MAX_SIDE || w_in < 1 || w_in > BL_MAX_SIDE ||
        !baseline_sizes_ok(n_case, h_out, w_out))
        return fail(CAE_ERR_ARG, "cae_case_baseline: bad argument (CAE_ELEM_* kinds, a CAE_INTERP_* mode, n_case >= 0, sides of 1 to 2^30)");
    if (L.stride < 0 || A.stride < 0 || (P.p && P.stride < 0)) return fail(CAE_ERR_ARG, "cae_case_baseline: negative stride");
    if (n_case == 0) return CAE_OK;
    const int64_t plane_in = h_in * w_in, plane = h_out * w_out;
    if (!L.p || !A.p || !sums) return fail(CAE_ERR_ARG, "cae_case_baseline: null pointer");
    if (shorter(L, plane_in) || shorter(A, plane) || (P.p && shorter(P, plane)))
        return fail(CAE_ERR_ARG, "cae_case_baseline: a case stride is shorter than the plane");
    if (reaches(L, n_case, plane_in) || reaches(A, n_case, plane) || (P.p && reaches(P, n_case, plane)) ||
        (field && (__int128)n_case * plane > ((__int128)1 << 60)))
        return fail(CAE_ERR_ARG, "cae_case_baseline: an operand reaches 2^60 elements from its pointer");
    if (misaligned(L) || misaligned(A) || (P.p && misaligned(P)) || ((uintptr_t)sums & 7) || ((uintptr_t)field & 7) ||
        ((uintptr_t)workspace & 7))
        return fail(CAE_ERR_ARG, "cae_case_baseline: pointers must be aligned to their element size, the workspace to 8 bytes");
    const int64_t need = cae_case_baseline_workspace_bytes(n_case, h_out, w_out);
    if (!workspace || workspace_bytes < need)
        return fail(CAE_ERR_ARG, "cae_case_baseline: needs a workspace of %lld bytes (cae_case_baseline_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)hip_stream;
    BlArgs a;
    memset(&a, 0, sizeof a);
    a.low = (const unsigned char*)low, a.p = (const unsigned char*)pred, a.a = (const unsigned char*)actual;
    a.low_stride = low_stride, a.p_stride = pred ? pred_stride : 0, a.a_stride = actual_stride;
    a.lk = low_kind, a.pk = pred ? pred_kind : 0, a.ak = actual_kind;
    a.h_in = (int)h_in, a.w_in = (int)w_in, a.h_out = (int)h_out, a.w_out = (int)w_out;
    a.sy = (double)h_in / (double)h_out, a.sx = (double)w_in / (double)w_out;
    a.n_band = (int)((h_out + BL_ROWS - 1) / BL_ROWS), a.n_strip = (int)((w_out + BL_COLS - 1) / BL_COLS);
    a.items = n_case * baseline_items(h_out, w_out);
    a.part = (double*)workspace, a.field = field;
    if (!pred) a.pk = a.ak;                 // read as a second a, never used
    const dim3 grid((unsigned)((a.items + 3) / 4));
    const int ea = elem_bytes(a.ak), ep = elem_bytes(a.pk);
#define BL_LAUNCH(MODE)                                                                                      \
    if (ea == 4 && ep == 4) hipLaunchKernelGGL((k_case_baseline<MODE, 4, 4>), grid, dim3(256), 0, s, a);      \
    else if (ea == 4) hipLaunchKernelGGL((k_case_baseline<MODE, 4, 8>), grid, dim3(256), 0, s, a);            \
    else if (ep == 4) hipLaunchKernelGGL((k_case_baseline<MODE, 8, 4>), grid, dim3(256), 0, s, a);            \
    else hipLaunchKernelGGL((k_case_baseline<MODE, 8, 8>), grid, dim3(256), 0, s, a);
    switch (mode) {
    case CAE_INTERP_NEAREST: BL_LAUNCH(0) break;
    case CAE_INTERP_BILINEAR: BL_LAUNCH(1) break;
    default: BL_LAUNCH(2) break;
    }
#undef BL_LAUNCH
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_baseline_fold, dim3((unsigned)ceil_capped(n_case * BL_SUMS, 256, 4096)), dim3(256), 0, s,
                       (const double*)workspace, (long long)n_case, (int)baseline_items(h_out, w_out), sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- a box model applied to a whole scene: tiles out, blended scene back ---------------------------------

// tiles along an axis of `extent` pixels for a box side and an overlap: 1 + ceil((extent - box) / (box - overlap))
static int64_t scene_tiles_along(int64_t extent, int box, int overlap) {
    const int64_t s = box - overlap;
    return 1 + (extent - box + s - 1) / s;
}

static int scene_geom_check(const char* who, const cae_scene_geom* g, bool with_scale) {
    if (!g) return fail(CAE_ERR_ARG, "%s: null geometry", who);
    if (g->h < 1 || g->w < 1 || g->Y < g->h || g->X < g->w || g->Y > ((int64_t)1 << 30) || g->X > ((int64_t)1 << 30))
        return fail(CAE_ERR_ARG, "%s: a scene of %lld x %lld pixels does not hold a box of %d x %d (sides up to 2^30)", who,
                    (long long)g->Y, (long long)g->X, g->h, g->w);
    if (g->oy < 0 || g->oy >= g->h || g->ox < 0 || g->ox >= g->w)
        return fail(CAE_ERR_ARG, "%s: the overlap (%d, %d) must be at least 0 and below the box (%d, %d)", who, g->oy, g->ox, g->h, g->w);
    if (with_scale) {
        if (g->sy < 1 || g->sx < 1) return fail(CAE_ERR_ARG, "%s: the scale (%d, %d) must be at least 1", who, g->sy, g->sx);
        if ((__int128)4 * g->h * g->sy * g->w * g->sx >= ((__int128)1 << 29))
            return fail(CAE_ERR_ARG, "%s: 4 H W must stay below 2^29 (the weights times an fp32 value are then exact in fp64)", who);
    }
    return CAE_OK;
}

int cae_scene_gather(const cae_scene_geom* geom, const void* src, int src_kind, int64_t n_t, int c_src, int64_t t0,
                     int64_t n_t_call, int64_t ky0, int64_t n_ky, float* dst, int c_dst, int c_off, float vmin, float range,
                     int enable, int32_t* invalid, void* hip_stream) {
    const int rc = scene_geom_check("cae_scene_gather", geom, false);
    if (rc != CAE_OK) return rc;
    if (!kind_known(src_kind) || n_t < 0 || c_src < 1 || c_off < 0 || c_off > c_dst - c_src ||
        t0 < 0 || n_t_call < 0 || t0 > n_t - n_t_call || ky0 < 0 || n_ky < 0)
        return fail(CAE_ERR_ARG, "cae_scene_gather: bad argument (a CAE_ELEM_* kind, the time range inside the variable, the channels inside the batch)");
    const int64_t n_y = scene_tiles_along(geom->Y, geom->h, geom->oy), n_x = scene_tiles_along(geom->X, geom->w, geom->ox);
    if (ky0 > n_y - n_ky) return fail(CAE_ERR_ARG, "cae_scene_gather: tile rows %lld .. %lld of %lld", (long long)ky0,
                                      (long long)(ky0 + n_ky), (long long)n_y);
    if (n_t_call == 0 || n_ky == 0) return CAE_OK;
    if (!src || !dst || !invalid) return fail(CAE_ERR_ARG, "cae_scene_gather: null pointer");
    if (((uintptr_t)src % elem_bytes(src_kind)) || ((uintptr_t)dst & 3) || ((uintptr_t)invalid & 3))
        return fail(CAE_ERR_ARG, "cae_scene_gather: pointers must be aligned to their element size");
    const __int128 per = (__int128)c_src * geom->h * geom->w, tiles = (__int128)n_t_call * n_ky * n_x;
    if (per > 0x7fffffffLL || (__int128)c_dst * geom->h * geom->w > 0x7fffffffLL || tiles > 0x7fffffffLL ||
        tiles * c_dst * geom->h * geom->w > ((__int128)1 << 60) || (__int128)n_t * c_src * geom->Y * geom->X > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_scene_gather: too large (2^31 - 1 tiles and box elements, 2^60 elements per operand)");
    SgArgs a;
    memset(&a, 0, sizeof a);
    a.src = (const unsigned char*)src, a.Y = geom->Y, a.X = geom->X, a.c_src = c_src, a.h = geom->h, a.w = geom->w;
    a.stride_y = geom->h - geom->oy, a.stride_x = geom->w - geom->ox, a.n_x = n_x;
    a.t0 = t0, a.ky0 = ky0, a.n_ky = n_ky, a.total = (long long)(tiles * per);
    a.dst = dst, a.c_dst = c_dst, a.c_off = c_off, a.vmin = vmin, a.range = range, a.enable = enable, a.invalid = (int*)invalid;
    const dim3 grid((unsigned)ceil_capped(a.total, 256 * 4, 8192));
    hipStream_t s = (hipStream_t)hip_stream;
    with_kind(src_kind, [&](auto KS) { hipLaunchKernelGGL((k_scene_gather<decltype(KS)::value>), grid, dim3(256), 0, s, a); });
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_scene_blend(const cae_scene_geom* geom, const float* pred, const int32_t* invalid, int64_t k0, int64_t n_k,
                    const float* carry_pred, const int32_t* carry_invalid, int64_t carry_k0, int64_t carry_n_k,
                    int64_t n_t_call, int c_out, int64_t row0, int64_t row1, double vmin, double range, double* out,
                    int64_t out_t_stride, int64_t* nan_pixels, void* hip_stream) {
    const int rc = scene_geom_check("cae_scene_blend", geom, true);
    if (rc != CAE_OK) return rc;
    const int64_t n_y = scene_tiles_along(geom->Y, geom->h, geom->oy), n_x = scene_tiles_along(geom->X, geom->w, geom->ox);
    const int64_t H = (int64_t)geom->h * geom->sy, W = (int64_t)geom->w * geom->sx;
    const int64_t Ys = geom->Y * geom->sy, Xs = geom->X * geom->sx;
    if (Ys > ((int64_t)1 << 30) || Xs > ((int64_t)1 << 30))
        return fail(CAE_ERR_ARG, "cae_scene_blend: an output of %lld x %lld pixels (sides up to 2^30)", (long long)Ys, (long long)Xs);
    if (n_t_call < 0 || c_out < 1 || k0 < 0 || n_k < 0 || k0 > n_y - n_k || carry_n_k < 0 || carry_k0 < 0 || carry_k0 > n_y - carry_n_k ||
        row0 < 0 || row1 < row0 || row1 > Ys || out_t_stride < 0 || (n_t_call > 1 && out_t_stride < (__int128)c_out * Ys * Xs))
        return fail(CAE_ERR_ARG, "cae_scene_blend: bad argument (tile rows inside the scene's %lld, output rows inside its %lld, "
                                 "a time stride of at least a scene)", (long long)n_y, (long long)Ys);
    if (carry_n_k > 0 && carry_k0 + carry_n_k > k0)
        return fail(CAE_ERR_ARG, "cae_scene_blend: the carried tile rows must come before the new ones");
    if (n_t_call == 0 || row1 == row0) return CAE_OK;
    if (n_t_call * c_out > 65535) return fail(CAE_ERR_ARG, "cae_scene_blend: more than 65535 (time step, channel) planes in a call");
    if (!pred || !invalid || !out || !nan_pixels || (carry_n_k > 0 && (!carry_pred || !carry_invalid)))
        return fail(CAE_ERR_ARG, "cae_scene_blend: null pointer");
    if (((uintptr_t)pred & 3) || ((uintptr_t)invalid & 3) || ((uintptr_t)carry_pred & 3) || ((uintptr_t)carry_invalid & 3) ||
        ((uintptr_t)out & 7) || ((uintptr_t)nan_pixels & 7))
        return fail(CAE_ERR_ARG, "cae_scene_blend: pointers must be aligned to their element size");
    const __int128 limit = (__int128)1 << 60;
    if ((__int128)n_t_call * (n_k > carry_n_k ? n_k : carry_n_k) * n_x * c_out * H * W > limit ||
        (__int128)(n_t_call - 1) * out_t_stride + (__int128)c_out * Ys * Xs > limit)
        return fail(CAE_ERR_ARG, "cae_scene_blend: an operand reaches 2^60 elements from its pointer");
    // every tile row that covers an output row of the call must be in one of the two runs
    const int64_t SY = (int64_t)(geom->h - geom->oy) * geom->sy, LY = (geom->Y - geom->h) * geom->sy;
    auto origin = [&](int64_t k) { return k * SY < LY ? k * SY : LY; };
    for (int64_t k = 0; k < n_y; k++) {
        if (origin(k) + H <= row0 || origin(k) >= row1) continue;
        const bool here = (k >= k0 && k < k0 + n_k) || (k >= carry_k0 && k < carry_k0 + carry_n_k);
        if (!here) return fail(CAE_ERR_ARG, "cae_scene_blend: output rows %lld .. %lld need tile row %lld, which the call does not bring",
                               (long long)row0, (long long)row1, (long long)k);
    }
    SbArgs a;
    memset(&a, 0, sizeof a);
    a.pred_a = carry_pred, a.invalid_a = (const int*)carry_invalid, a.ka0 = (int)carry_k0, a.n_ka = (int)carry_n_k;
    a.pred_b = pred, a.invalid_b = (const int*)invalid, a.kb0 = (int)k0, a.n_kb = (int)n_k;
    a.n_y = (int)n_y, a.n_x = (int)n_x, a.n_t = (int)n_t_call, a.c_out = c_out, a.H = (int)H, a.W = (int)W;
    a.SY = (int)SY, a.SX = (geom->w - geom->ox) * geom->sx, a.LY = (int)LY, a.LX = (int)((geom->X - geom->w) * geom->sx);
    a.RY2 = 2 * geom->oy * geom->sy, a.RX2 = 2 * geom->ox * geom->sx;
    a.Xs = (int)Xs, a.row0 = (int)row0, a.row1 = (int)row1, a.out_c_stride = Ys * Xs, a.out_t_stride = out_t_stride;
    a.vmin = vmin, a.range = range, a.out = out, a.nan_pixels = (unsigned long long*)nan_pixels;
    // a workgroup per 256 columns and band of rows: about 8192 workgroups in all where the call is large enough
    const int64_t gx = (Xs + 255) / 256, gz = n_t_call * c_out, rows = row1 - row0;
    int64_t gy = 8192 / (gx * gz);
    gy = gy < 1 ? 1 : (gy > rows ? rows : gy);
    a.band = (int)((rows + gy - 1) / gy);
    gy = (rows + a.band - 1) / a.band;
    hipLaunchKernelGGL((k_scene_blend<SB_ROWS>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), 0, (hipStream_t)hip_stream, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- value distributions: joint histogram of prediction against target ------------------------------------
// (the last sections: their kernels are emitted after every other kernel of the code object)

static bool hist_sizes_ok(int64_t n_case, int64_t plane, int n_bin, int sub) {
    return n_case >= 0 && plane >= 0 && n_bin >= 1 && n_bin <= JH_MAX_BIN && sub >= 1 && sub <= JH_MAX_SUB &&
           (__int128)n_case * plane < ((__int128)1 << 40);
}

// the workgroups of a call, from (n_case, plane) alone: one per JH_WAVES items of cae_case_measures' cut, at most JH_MAX_GROUPS
static int64_t hist_groups(int64_t n_case, int64_t plane) { return ceil_capped(n_case * case_chunks(plane), JH_WAVES, JH_MAX_GROUPS); }

int64_t cae_joint_hist_workspace_bytes(int64_t n_case, int64_t plane, int n_bin, int sub) {
    if (n_case < 1 || plane < 1 || !hist_sizes_ok(n_case, plane, n_bin, sub)) return 0;
    return hist_groups(n_case, plane) * 2 * n_bin * 4 * (int64_t)sizeof(double);
}

extern "C++" {

template <int KP, int KA>
static void launch_joint_hist(dim3 grid, size_t lds, hipStream_t s, const JhArgs& a) {
    static size_t granted = 64 * 1024;      // above it a kernel has to ask
    if (lds > granted) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_joint_hist<KP, KA>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        granted = lds;
    }
    hipLaunchKernelGGL((k_joint_hist<KP, KA>), grid, dim3(64 * JH_WAVES), lds, s, a);
}

}  // extern "C++"

int cae_joint_hist(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                   int64_t actual_stride, int64_t n_case, int64_t plane, double lo, double hi, int n_bin, int sub,
                   int64_t* joint, int64_t* marg, double* cond, int64_t* outside, void* workspace, int64_t workspace_bytes,
                   void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!known(P) || !known(A) || !hist_sizes_ok(n_case, plane, n_bin, sub))
        return fail(CAE_ERR_ARG, "cae_joint_hist: bad argument (CAE_ELEM_* kinds, n_case >= 0, plane >= 0, 1 <= n_bin <= %d, "
                                 "1 <= sub <= %d, n_case * plane < 2^40)", JH_MAX_BIN, JH_MAX_SUB);
    const int n_fine = n_bin * sub;
    const double scale = (double)n_fine / (hi - lo);
    if (!(lo - lo == 0.0) || !(hi - hi == 0.0) || !(hi > lo) || !(scale - scale == 0.0) || !(scale > 0.0))
        return fail(CAE_ERR_ARG, "cae_joint_hist: lo and hi must be finite, hi > lo, and n_bin * sub / (hi - lo) finite and not zero");
    if (P.stride < 0 || A.stride < 0) return fail(CAE_ERR_ARG, "cae_joint_hist: negative stride");
    if (((uintptr_t)joint & 7) || ((uintptr_t)marg & 7) || ((uintptr_t)cond & 7) || ((uintptr_t)outside & 7))
        return fail(CAE_ERR_ARG, "cae_joint_hist: the outputs must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t joint_bytes = (size_t)n_bin * n_bin * sizeof(int64_t), marg_bytes = (size_t)2 * n_fine * sizeof(int64_t),
                 cond_bytes = (size_t)2 * n_bin * 4 * sizeof(double), outside_bytes = 4 * sizeof(int64_t);
    if (n_case == 0 || plane == 0) {        // no pixel, no pair: the outputs that are given are zeroed, no operand is looked at
        if (joint) HIP_TRY(hipMemsetAsync(joint, 0, joint_bytes, s));
        if (marg) HIP_TRY(hipMemsetAsync(marg, 0, marg_bytes, s));
        if (cond) HIP_TRY(hipMemsetAsync(cond, 0, cond_bytes, s));
        if (outside) HIP_TRY(hipMemsetAsync(outside, 0, outside_bytes, s));
        return CAE_OK;
    }
    if (!P.p || !A.p || !joint || !marg || !cond || !outside) return fail(CAE_ERR_ARG, "cae_joint_hist: null pointer");
    if (shorter(P, plane) || shorter(A, plane))
        return fail(CAE_ERR_ARG, "cae_joint_hist: a case stride is shorter than the plane");
    if (reaches(P, n_case, plane) || reaches(A, n_case, plane))
        return fail(CAE_ERR_ARG, "cae_joint_hist: an operand reaches 2^60 elements from its pointer");
    if (misaligned(P) || misaligned(A))
        return fail(CAE_ERR_ARG, "cae_joint_hist: pointers must be aligned to their element size");
    const int64_t need = cae_joint_hist_workspace_bytes(n_case, plane, n_bin, sub);
    if (workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_joint_hist: needs a workspace of %lld bytes (cae_joint_hist_workspace_bytes)", (long long)need);
    const int64_t n_group = hist_groups(n_case, plane);
    const int per = 2 * n_bin * 4;
    JhArgs a;
    memset(&a, 0, sizeof a);
    a.p = (const unsigned char*)P.p, a.a = (const unsigned char*)A.p;
    a.p_stride = P.stride, a.a_stride = A.stride, a.plane = plane;
    a.nch = (int)case_chunks(plane), a.items = n_case * case_chunks(plane);
    a.lo = lo, a.hi = hi, a.scale = scale;
    a.n_bin = n_bin, a.sub = sub, a.n_fine = n_fine;
    a.magic = (unsigned)(((1u << JH_SHIFT) + sub - 1) / sub);
    a.joint = (unsigned long long*)joint, a.marg = (unsigned long long*)marg, a.outside = (unsigned long long*)outside;
    a.part = (double*)workspace;
    HIP_TRY(hipMemsetAsync(joint, 0, joint_bytes, s));
    HIP_TRY(hipMemsetAsync(marg, 0, marg_bytes, s));
    HIP_TRY(hipMemsetAsync(outside, 0, outside_bytes, s));
    const size_t lds = (size_t)JH_WAVES * per * sizeof(double) + ((size_t)n_bin * n_bin + 2 * (size_t)n_fine) * sizeof(unsigned);
    const dim3 grid((unsigned)n_group);
    with_kind(P.kind, [&](auto KP) {
        with_kind(A.kind, [&](auto KA) { launch_joint_hist<decltype(KP)::value, decltype(KA)::value>(grid, lds, s, a); });
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_joint_hist_fold<JH_WAVES>), dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, (const double*)workspace,
                       (int)n_group, per, cond);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- skill by stratum: the error sums conditioned on a third field --------------------------------------

static bool strata_sizes_ok(int64_t n_case, int64_t h, int64_t w, int n_strata) {
    return n_case >= 0 && h >= 0 && h <= ST_MAX_SIDE && w >= 0 && w <= ST_MAX_SIDE && n_strata >= 1 && n_strata <= ST_MAX_STRATA;
}

static int64_t strata_chunks(int64_t plane) { return (plane + ST_CHUNK - 1) / ST_CHUNK; }

// the workgroups of a call, from (n_case, h, w) alone: one per ST_WAVES items, at most ST_MAX_GROUPS
static int64_t strata_groups(int64_t n_case, int64_t plane) {
    const __int128 items = (__int128)n_case * strata_chunks(plane);
    return items >= (__int128)ST_WAVES * ST_MAX_GROUPS ? ST_MAX_GROUPS : ceil_capped((int64_t)items, ST_WAVES, ST_MAX_GROUPS);
}

int64_t cae_strata_sums_workspace_bytes(int64_t n_case, int64_t h, int64_t w, int n_strata) {
    if (n_case < 1 || h < 1 || w < 1 || !strata_sizes_ok(n_case, h, w, n_strata)) return 0;
    return strata_groups(n_case, h * w) * n_strata * ST_SUMS * (int64_t)sizeof(double);
}

int cae_strata_sums(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                    int64_t actual_stride, const void* strata, int strata_kind, int64_t strata_stride, int64_t n_case,
                    int64_t h, int64_t w, int64_t sh, int64_t sw, const double* edges, int n_edge, const double* shift_a,
                    const double* shift_p, int64_t* counts, double* sums, void* workspace, int64_t workspace_bytes,
                    void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride}, S{strata, strata_kind, strata_stride};
    if (!known(P) || !known(A) || !known(S) || n_edge < 0 || n_edge > ST_MAX_EDGE || !strata_sizes_ok(n_case, h, w, n_edge + 1) ||
        sh < 1 || sh > ST_MAX_SIDE || sw < 1 || sw > ST_MAX_SIDE)
        return fail(CAE_ERR_ARG, "cae_strata_sums: bad argument (CAE_ELEM_* kinds, n_case >= 0, target sides of 0 to 2^30, "
                                 "stratifier sides of 1 to 2^30, 0 <= n_edge <= %d)", ST_MAX_EDGE);
    if (P.stride < 0 || A.stride < 0 || S.stride < 0) return fail(CAE_ERR_ARG, "cae_strata_sums: negative stride");
    if (((uintptr_t)counts & 7) || ((uintptr_t)sums & 7)) return fail(CAE_ERR_ARG, "cae_strata_sums: the outputs must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const int n_strata = n_edge + 1;
    const size_t counts_bytes = (size_t)(2 * n_strata + 1) * sizeof(int64_t), sums_bytes = (size_t)n_strata * ST_SUMS * sizeof(double);
    if (n_case == 0 || h == 0 || w == 0) {  // no pixel: the outputs that are given are zeroed, no operand is looked at
        if (counts) HIP_TRY(hipMemsetAsync(counts, 0, counts_bytes, s));
        if (sums) HIP_TRY(hipMemsetAsync(sums, 0, sums_bytes, s));
        return CAE_OK;
    }
    if (!P.p || !A.p || !S.p || !counts || !sums || (n_edge > 0 && !edges) || !shift_a || !shift_p)
        return fail(CAE_ERR_ARG, "cae_strata_sums: null pointer");
    for (int j = 0; j < n_edge; j++)
        if (!(edges[j] - edges[j] == 0.0) || (j > 0 && !(edges[j] > edges[j - 1])))
            return fail(CAE_ERR_ARG, "cae_strata_sums: the edges must be finite and strictly ascending");
    for (int k = 0; k < n_strata; k++)
        if (!(shift_a[k] - shift_a[k] == 0.0) || !(shift_p[k] - shift_p[k] == 0.0))
            return fail(CAE_ERR_ARG, "cae_strata_sums: the shifts must be finite");
    const int64_t plane = h * w, plane_s = sh * sw;
    if (shorter(P, plane) || shorter(A, plane) || shorter(S, plane_s))
        return fail(CAE_ERR_ARG, "cae_strata_sums: a case stride is shorter than the plane");
    if (reaches(P, n_case, plane) || reaches(A, n_case, plane) || reaches(S, n_case, plane_s))
        return fail(CAE_ERR_ARG, "cae_strata_sums: an operand reaches 2^60 elements from its pointer");
    if (misaligned(P) || misaligned(A) || misaligned(S))
        return fail(CAE_ERR_ARG, "cae_strata_sums: pointers must be aligned to their element size");
    const int64_t need = cae_strata_sums_workspace_bytes(n_case, h, w, n_strata);
    if (workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_strata_sums: needs a workspace of %lld bytes (cae_strata_sums_workspace_bytes)", (long long)need);
    const int64_t n_group = strata_groups(n_case, plane);
    const int per = n_strata * ST_SUMS;
    StArgs a;
    memset(&a, 0, sizeof a);
    a.p = (const unsigned char*)P.p, a.a = (const unsigned char*)A.p, a.s = (const unsigned char*)S.p;
    a.p_stride = P.stride, a.a_stride = A.stride, a.s_stride = S.stride, a.sk = S.kind;
    a.h = (int)h, a.w = (int)w, a.sh = (int)sh, a.sw = (int)sw;
    a.q64 = (int)(64 / w), a.r64 = (int)(64 % w), a.n_edge = n_edge;
    a.sy = (double)sh / (double)h, a.sx = (double)sw / (double)w;
    a.plane = plane, a.nch = strata_chunks(plane), a.items = n_case * a.nch;
    a.counts = (unsigned long long*)counts, a.part = (double*)workspace;
    for (int j = 0; j < n_edge; j++) a.edges[j] = edges[j];
    for (int k = 0; k < n_strata; k++) a.shift_a[k] = shift_a[k], a.shift_p[k] = shift_p[k];
    HIP_TRY(hipMemsetAsync(counts, 0, counts_bytes, s));
    const dim3 grid((unsigned)n_group);
    with_kind(P.kind, [&](auto KP) {
        with_kind(A.kind, [&](auto KA) {
            hipLaunchKernelGGL((k_strata_sums<decltype(KP)::value, decltype(KA)::value>), grid, dim3(64 * ST_WAVES), 0, s, a);
        });
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_strata_fold<ST_WAVES>), dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, (const double*)workspace,
                       (int)n_group, per, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- neighbourhood skill: the window sums of the Fractions Skill Score ---------------------------------

static bool fss_sizes_ok(int64_t n_case, int64_t h, int64_t w, int n_thr) {
    return n_case >= 0 && n_case <= FS_MAX_CASES && h >= 0 && h <= FS_MAX_SIDE && w >= 0 && w <= FS_MAX_SIDE && n_thr >= 1 &&
           n_thr <= FS_MAX_THR;
}

// the bit-planes of a call in bytes, INT64_MAX where they pass it (no workspace is that large: the call is then refused)
static int64_t fss_plane_bytes(int64_t n_case, int64_t h, int64_t w, int n_thr) {
    const __int128 bytes = (__int128)n_case * (1 + 2 * n_thr) * h * ((w + 63) / 64) * 8;
    return bytes > (__int128)INT64_MAX ? INT64_MAX : (int64_t)bytes;
}

// The window rows of a segment of k_fss_windows.  A segment first adds its first n rows, so a long one keeps that start-up
// small - 129 rows before 512 steps at the widest neighbourhood - and a short one gives a small call more waves: halved
// while the call has fewer than 4096 items and the segment more than 64 rows.  Integer sums: the cut never shows.
static int fss_seg_len(int64_t n_case, int64_t h, int64_t wpr, int n_thr) {
    int len = 512;
    while (len > 64 && (__int128)n_case * n_thr * wpr * ((h + len - 1) / len) < 4096) len /= 2;
    return len;
}

int64_t cae_case_fss_workspace_bytes(int64_t n_case, int64_t h, int64_t w, int n_thr) {
    if (n_case < 1 || h < 1 || w < 1 || !fss_sizes_ok(n_case, h, w, n_thr)) return 0;
    return fss_plane_bytes(n_case, h, w, n_thr);
}

int cae_case_fss(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind, int64_t actual_stride,
                 int64_t n_case, int64_t h, int64_t w, const double* thresholds, const int* sides, int n_thr, const int* widths,
                 int n_width, int gap_rule, int64_t* sums, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride};
    if (!known(P) || !known(A) || !fss_sizes_ok(n_case, h, w, n_thr) || n_width < 1 || n_width > FS_MAX_WIDTH ||
        (gap_rule != 0 && gap_rule != 1))
        return fail(CAE_ERR_ARG, "cae_case_fss: bad argument (CAE_ELEM_* kinds, 0 <= n_case <= 2^40, sides of 0 to %lld, 1 <= n_thr <= %d, "
                                 "1 <= n_width <= %d, gap_rule 0 or 1)", FS_MAX_SIDE, FS_MAX_THR, FS_MAX_WIDTH);
    if (P.stride < 0 || A.stride < 0) return fail(CAE_ERR_ARG, "cae_case_fss: negative stride");
    if ((uintptr_t)sums & 7) return fail(CAE_ERR_ARG, "cae_case_fss: the output must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t sums_bytes = (size_t)n_case * n_thr * n_width * FS_SUMS * sizeof(int64_t);
    if (n_case == 0 || h == 0 || w == 0) {  // no window: the output that is given is zeroed, no operand is looked at
        if (sums && sums_bytes) HIP_TRY(hipMemsetAsync(sums, 0, sums_bytes, s));
        return CAE_OK;
    }
    if (!P.p || !A.p || !thresholds || !sides || !widths || !sums) return fail(CAE_ERR_ARG, "cae_case_fss: null pointer");
    for (int t = 0; t < n_thr; t++)
        if (!(thresholds[t] - thresholds[t] == 0.0)) return fail(CAE_ERR_ARG, "cae_case_fss: the thresholds must be finite");
    for (int t = 0; t < n_thr; t++)
        if (sides[t] != 0 && sides[t] != 1) return fail(CAE_ERR_ARG, "cae_case_fss: a side must be 0 (above) or 1 (below)");
    for (int j = 0; j < n_width; j++)
        if (widths[j] < 1 || widths[j] > FS_MAX_N || widths[j] % 2 == 0 || (j > 0 && widths[j] <= widths[j - 1]))
            return fail(CAE_ERR_ARG, "cae_case_fss: the widths must be odd, from 1 to %d and strictly ascending", FS_MAX_N);
    const int64_t plane = h * w;
    if (shorter(P, plane) || shorter(A, plane)) return fail(CAE_ERR_ARG, "cae_case_fss: a case stride is shorter than the plane");
    if (reaches(P, n_case, plane) || reaches(A, n_case, plane))
        return fail(CAE_ERR_ARG, "cae_case_fss: an operand reaches 2^60 elements from its pointer");
    if (misaligned(P) || misaligned(A)) return fail(CAE_ERR_ARG, "cae_case_fss: pointers must be aligned to their element size");
    const int64_t need = cae_case_fss_workspace_bytes(n_case, h, w, n_thr);
    if (workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_case_fss: needs a workspace of %lld bytes (cae_case_fss_workspace_bytes)", (long long)need);
    const int64_t wpr = (w + 63) / 64;
    FsBitsArgs b;
    memset(&b, 0, sizeof b);
    b.p = (const unsigned char*)P.p, b.a = (const unsigned char*)A.p, b.p_stride = P.stride, b.a_stride = A.stride;
    b.h = (int)h, b.w = (int)w, b.wpr = (int)wpr, b.n_thr = n_thr, b.words = n_case * h * wpr;
    b.planes = (unsigned long long*)workspace;
    for (int t = 0; t < n_thr; t++) b.thr[t] = thresholds[t], b.below[t] = sides[t];
    FsWinArgs g;
    memset(&g, 0, sizeof g);
    g.h = (int)h, g.w = (int)w, g.wpr = (int)wpr, g.n_thr = n_thr, g.n_width = n_width, g.gap_rule = gap_rule;
    g.seg_len = fss_seg_len(n_case, h, wpr, n_thr), g.n_seg = (int)((h + g.seg_len - 1) / g.seg_len);
    g.items = n_case * n_thr * g.n_seg * wpr;
    for (int j = 0; j < n_width; j++) g.width[j] = widths[j];
    HIP_TRY(hipMemsetAsync(sums, 0, sums_bytes, s));
    const dim3 grid_b((unsigned)ceil_capped(b.words, FS_WAVES * FS_AHEAD, FS_BITS_GROUPS));
    with_kind(P.kind, [&](auto KP) {
        with_kind(A.kind, [&](auto KA) {
            hipLaunchKernelGGL((k_fss_bits<decltype(KP)::value, decltype(KA)::value>), grid_b, dim3(64 * FS_WAVES), 0, s, b);
        });
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_fss_windows<FS_WAVES>), dim3((unsigned)ceil_capped(g.items, FS_WAVES, FS_WIN_GROUPS)), dim3(64 * FS_WAVES), 0,
                       s, (const unsigned long long*)workspace, (unsigned long long*)sums, g);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- permutation importance: a batch with rows drawn from other cases, and the comparison of its scores -----------

int cae_normalise_pack_gather(const float* src, int64_t n_src, int c_src, int64_t hw, float* dst, int64_t n_dst, int c_dst, int c_off,
                              float vmin, float range, int enable, const int32_t* row_dev, void* hip_stream) {
    if (n_src < 0 || n_dst < 0 || c_src < 1 || hw < 0 || c_off < 0 || c_off > c_dst - c_src)
        return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: bad argument (n_src >= 0, n_dst >= 0, c_src >= 1, hw >= 0, "
                                 "0 <= c_off <= c_dst - c_src)");
    if (n_src > 0x7fffffffLL || n_dst > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: more than 2^31 - 1 rows");
    if (n_dst == 0 || hw == 0) return CAE_OK;
    if ((!src && n_src > 0) || !dst || !row_dev) return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: null pointer");
    if ((__int128)n_src * c_src * hw > ((__int128)1 << 60) || (__int128)n_dst * c_dst * hw > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: an operand reaches 2^60 elements from its pointer");
    if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)row_dev & 3))
        return fail(CAE_ERR_ARG, "cae_normalise_pack_gather: pointers must be 4-byte aligned");
    const long long total = (long long)n_dst * c_src * hw;
    const int blocks = (int)ceil_capped(total, 256 * 8, 8192);
    hipLaunchKernelGGL((k_normalise_pack_gather<256>), dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, src, (long long)n_src, total,
                       c_src, (long long)hw, dst, c_dst, c_off, vmin, range, enable, (const int*)row_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

static int64_t importance_tiles(int64_t plane) { return (plane + IM_TILE - 1) / IM_TILE; }

int64_t cae_case_importance_workspace_bytes(int64_t n_case, int64_t plane) {
    if (n_case < 1 || plane < 1 || (__int128)n_case * plane > ((__int128)1 << 60)) return 0;
    return n_case * importance_tiles(plane) * IM_SUMS * (int64_t)sizeof(double);
}

int cae_case_importance(const float* base, int64_t base_stride, const float* pert, int64_t pert_stride, const void* actual,
                        int actual_kind, int64_t actual_stride, int64_t n_case, int64_t plane, double vmin, double range,
                        double* sums, double* map, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand B{base, CAE_ELEM_F32, base_stride}, Q{pert, CAE_ELEM_F32, pert_stride}, A{actual, actual_kind, actual_stride};
    if (!known(A) || n_case < 0 || plane < 0)
        return fail(CAE_ERR_ARG, "cae_case_importance: bad argument (a CAE_ELEM_* kind, n_case >= 0, plane >= 0)");
    if (B.stride < 0 || Q.stride < 0 || A.stride < 0) return fail(CAE_ERR_ARG, "cae_case_importance: negative stride");
    if (!(vmin - vmin == 0.0) || !(range - range == 0.0)) return fail(CAE_ERR_ARG, "cae_case_importance: vmin and range must be finite");
    if (n_case == 0 || plane == 0) return CAE_OK;
    if (!B.p || !Q.p || !A.p || !sums) return fail(CAE_ERR_ARG, "cae_case_importance: null pointer");
    if (shorter(B, plane) || shorter(Q, plane) || shorter(A, plane))
        return fail(CAE_ERR_ARG, "cae_case_importance: a case stride is shorter than the plane");
    if (reaches(B, n_case, plane) || reaches(Q, n_case, plane) || reaches(A, n_case, plane) ||
        (__int128)n_case * plane > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_case_importance: an operand reaches 2^60 elements from its pointer");
    if (misaligned(B) || misaligned(Q) || misaligned(A) || ((uintptr_t)sums & 7) || ((uintptr_t)map & 7) || ((uintptr_t)workspace & 15))
        return fail(CAE_ERR_ARG, "cae_case_importance: pointers must be aligned to their element size, the workspace to 16 bytes");
    const int64_t need = cae_case_importance_workspace_bytes(n_case, plane);
    if (!workspace || workspace_bytes < need)
        return fail(CAE_ERR_ARG, "cae_case_importance: needs a workspace of %lld bytes (cae_case_importance_workspace_bytes)", (long long)need);
    hipStream_t s = (hipStream_t)hip_stream;
    ImArgs a;
    memset(&a, 0, sizeof a);
    a.base = base, a.pert = pert, a.a = (const unsigned char*)actual;
    a.base_stride = base_stride, a.pert_stride = pert_stride, a.a_stride = actual_stride;
    a.n_case = n_case, a.plane = plane, a.n_tile = importance_tiles(plane);
    a.items = map ? a.n_tile : a.n_tile * ((n_case + IM_RUN - 1) / IM_RUN);
    a.vmin = vmin, a.range = range, a.part = (double*)workspace, a.map = map;
    const dim3 grid((unsigned)ceil_capped(a.items, IM_WAVES, map ? (int64_t)1 << 20 : 16384));
    with_kind(A.kind, [&](auto KA) {
        if (map) hipLaunchKernelGGL((k_case_importance<decltype(KA)::value, true>), grid, dim3(64 * IM_WAVES), 0, s, a);
        else hipLaunchKernelGGL((k_case_importance<decltype(KA)::value, false>), grid, dim3(64 * IM_WAVES), 0, s, a);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_importance_fold<IM_WAVES>), dim3((unsigned)ceil_capped(n_case, IM_WAVES, 8192)), dim3(64 * IM_WAVES), 0, s,
                       (const double*)workspace, (long long)n_case, (long long)a.n_tile, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- prediction intervals: exact order statistics of the absolute residual, the counts below them, the bounds -----------

static bool quantile_sizes_ok(int64_t n_case, int64_t plane, int group) {
    return n_case >= 0 && n_case <= 0x7fffffffLL && plane >= 0 && plane <= ((int64_t)1 << 40) &&
           (__int128)n_case * plane <= ((__int128)1 << 40) && (group == 0 || group == 1);
}

// The operand checks cae_score_quantiles and cae_score_counts share, after the sizes: S.p NULL stands for "no scale".
static int quantile_operand_check(const char* who, const CaseOperand& P, const CaseOperand& A, const CaseOperand& S, int64_t n_case,
                                  int64_t plane) {
    if (!P.p || !A.p) return fail(CAE_ERR_ARG, "%s: null pointer", who);
    if (shorter(P, plane) || shorter(A, plane) || (S.p && shorter(S, plane)))
        return fail(CAE_ERR_ARG, "%s: a case stride is shorter than the plane", who);
    if (reaches(P, n_case, plane) || reaches(A, n_case, plane) || (S.p && reaches(S, n_case, plane)))
        return fail(CAE_ERR_ARG, "%s: an operand reaches 2^60 elements from its pointer", who);
    if (misaligned(P) || misaligned(A) || (S.p && misaligned(S)))
        return fail(CAE_ERR_ARG, "%s: pointers must be aligned to their element size", who);
    return CAE_OK;
}

static void quantile_args(QtArgs& g, const CaseOperand& P, const CaseOperand& A, const CaseOperand& S, int64_t n_case, int64_t plane,
                          int n_level) {
    memset(&g, 0, sizeof g);
    g.p = (const unsigned char*)P.p, g.a = (const unsigned char*)A.p, g.s = (const unsigned char*)S.p;
    g.p_stride = P.stride, g.a_stride = A.stride, g.s_stride = S.p ? S.stride : 0;
    g.p_be = P.kind & 1, g.a_be = A.kind & 1, g.s_be = S.p ? S.kind & 1 : 0;
    g.n_level = n_level, g.n_case = n_case, g.plane = plane;
    g.n_tile = (plane + 63) / 64, g.total = n_case * plane;
}

extern "C++" {
// f(WP, WA, WS): the element widths of the three operands in bytes, 0 for a scale that is not there
template <class F>
static void with_widths(const CaseOperand& P, const CaseOperand& A, const CaseOperand& S, F&& f) {
    auto third = [&](auto WP, auto WA) {
        if (!S.p) f(WP, WA, std::integral_constant<int, 0>());
        else if (elem_bytes(S.kind) == 4) f(WP, WA, std::integral_constant<int, 4>());
        else f(WP, WA, std::integral_constant<int, 8>());
    };
    auto second = [&](auto WP) {
        if (elem_bytes(A.kind) == 4) third(WP, std::integral_constant<int, 4>());
        else third(WP, std::integral_constant<int, 8>());
    };
    if (elem_bytes(P.kind) == 4) second(std::integral_constant<int, 4>());
    else second(std::integral_constant<int, 8>());
}
}  // extern "C++"

static int64_t quantile_pool_bytes() { return (QT_POOL_STATE + QT_MAX_LEVELS * QT_POOL_BINS) * (int64_t)sizeof(unsigned long long); }
static int64_t quantile_pool_groups(int64_t total) { return ceil_capped((total + 63) / 64, 4 * QT_AHEAD, 2048); }

int64_t cae_score_quantiles_workspace_bytes(int64_t n_case, int64_t plane, int group, int n_level) {
    if (n_case < 1 || plane < 1 || !quantile_sizes_ok(n_case, plane, group) || n_level < 1 || n_level > QT_MAX_LEVELS) return 0;
    return group == 1 ? quantile_pool_bytes() : 0;
}

int cae_score_quantiles(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind,
                        int64_t actual_stride, const void* scale, int scale_kind, int64_t scale_stride, int64_t n_case,
                        int64_t plane, int group, const int64_t* num, const int64_t* den, int n_level, double* q, int64_t* n,
                        void* workspace, int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride},
        S{scale, scale ? scale_kind : CAE_ELEM_F32, scale ? scale_stride : 0};
    if (!known(P) || !known(A) || !known(S) || !quantile_sizes_ok(n_case, plane, group) || n_level < 1 || n_level > QT_MAX_LEVELS)
        return fail(CAE_ERR_ARG, "cae_score_quantiles: bad argument (CAE_ELEM_* kinds, 0 <= n_case < 2^31, plane >= 0, at most 2^40 "
                                 "scores, group 0 or 1, 1 <= n_level <= %d)", QT_MAX_LEVELS);
    if (P.stride < 0 || A.stride < 0 || S.stride < 0) return fail(CAE_ERR_ARG, "cae_score_quantiles: negative stride");
    if (!num || !den || !q || !n) return fail(CAE_ERR_ARG, "cae_score_quantiles: null pointer");
    for (int l = 0; l < n_level; l++)
        if (!(num[l] > 0 && num[l] < den[l] && den[l] <= 1000000) || (l > 0 && !(num[l - 1] * den[l] < num[l] * den[l - 1])))
            return fail(CAE_ERR_ARG, "cae_score_quantiles: the levels must be num / den with 0 < num < den <= 10^6, strictly ascending");
    if (((uintptr_t)q & 7) || ((uintptr_t)n & 7)) return fail(CAE_ERR_ARG, "cae_score_quantiles: the outputs must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t groups = group == 1 ? 1 : plane;
    if (n_case == 0 || plane == 0) {    // no score: every group that exists has n = 0 and q = +inf, no operand is looked at
        if (groups > 0) {
            hipLaunchKernelGGL((k_quantile_fill<256>), dim3((unsigned)ceil_capped(groups * n_level, 256, 4096)), dim3(256), 0, s, q,
                               (long long)(groups * n_level), __builtin_huge_val());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemsetAsync(n, 0, (size_t)groups * sizeof(int64_t), s));
        }
        return CAE_OK;
    }
    if (const int rc = quantile_operand_check("cae_score_quantiles", P, A, S, n_case, plane)) return rc;
    const int64_t need = cae_score_quantiles_workspace_bytes(n_case, plane, group, n_level);
    if (need > 0 && workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_score_quantiles: needs a workspace of %lld bytes (cae_score_quantiles_workspace_bytes)",
                    (long long)need);
    QtArgs g;
    quantile_args(g, P, A, S, n_case, plane, n_level);
    for (int l = 0; l < n_level; l++) g.num[l] = num[l], g.den[l] = den[l];
    g.q = q, g.n = (long long*)n;
    if (group == 0) {
        const dim3 grid((unsigned)(g.n_tile < ((int64_t)1 << 20) ? g.n_tile : ((int64_t)1 << 20)));
        const size_t lds = (size_t)n_level * QT_BINS * 64 * sizeof(unsigned);
        with_widths(P, A, S, [&](auto WP, auto WA, auto WS) {
            hipLaunchKernelGGL((k_quantile_pixel<decltype(WP)::value, decltype(WA)::value, decltype(WS)::value>), grid,
                               dim3(64 * QT_WAVES), lds, s, g);
        });
        HIP_TRY(hipGetLastError());
        return CAE_OK;
    }
    g.pool = (unsigned long long*)workspace;
    HIP_TRY(hipMemsetAsync(workspace, 0, (size_t)need, s));
    const dim3 grid((unsigned)quantile_pool_groups(g.total));
    for (int pass = 0; pass < QT_POOL_PASSES; pass++) {
        g.pass = pass;
        with_widths(P, A, S, [&](auto WP, auto WA, auto WS) {
            hipLaunchKernelGGL((k_quantile_pool_count<decltype(WP)::value, decltype(WA)::value, decltype(WS)::value>), grid, dim3(256),
                               0, s, g);
        });
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL((k_quantile_pool_scan<256>), dim3(1), dim3(256), 0, s, g);
        HIP_TRY(hipGetLastError());
    }
    return CAE_OK;
}

int cae_score_counts(const void* pred, int pred_kind, int64_t pred_stride, const void* actual, int actual_kind, int64_t actual_stride,
                     const void* scale, int scale_kind, int64_t scale_stride, int64_t n_case, int64_t plane, int group,
                     const double* q, int n_level, int64_t* count, int64_t* n, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, A{actual, actual_kind, actual_stride},
        S{scale, scale ? scale_kind : CAE_ELEM_F32, scale ? scale_stride : 0};
    if (!known(P) || !known(A) || !known(S) || !quantile_sizes_ok(n_case, plane, group) || n_level < 1 || n_level > QT_MAX_LEVELS)
        return fail(CAE_ERR_ARG, "cae_score_counts: bad argument (CAE_ELEM_* kinds, 0 <= n_case < 2^31, plane >= 0, at most 2^40 "
                                 "scores, group 0 or 1, 1 <= n_level <= %d)", QT_MAX_LEVELS);
    if (P.stride < 0 || A.stride < 0 || S.stride < 0) return fail(CAE_ERR_ARG, "cae_score_counts: negative stride");
    if (!count || !n) return fail(CAE_ERR_ARG, "cae_score_counts: null pointer");
    if (((uintptr_t)q & 7) || ((uintptr_t)count & 7) || ((uintptr_t)n & 7))
        return fail(CAE_ERR_ARG, "cae_score_counts: q and the outputs must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t groups = group == 1 ? 1 : plane;
    if (n_case == 0 || plane == 0) {    // no score: the counts of every group that exists are zero
        if (groups > 0) {
            HIP_TRY(hipMemsetAsync(count, 0, (size_t)groups * n_level * sizeof(int64_t), s));
            HIP_TRY(hipMemsetAsync(n, 0, (size_t)groups * sizeof(int64_t), s));
        }
        return CAE_OK;
    }
    if (!q) return fail(CAE_ERR_ARG, "cae_score_counts: null pointer");
    if (const int rc = quantile_operand_check("cae_score_counts", P, A, S, n_case, plane)) return rc;
    QtArgs g;
    quantile_args(g, P, A, S, n_case, plane, n_level);
    g.q_in = q, g.count = (unsigned long long*)count, g.n = (long long*)n;
    if (group == 0) {
        const dim3 grid((unsigned)(g.n_tile < ((int64_t)1 << 20) ? g.n_tile : ((int64_t)1 << 20)));
        with_widths(P, A, S, [&](auto WP, auto WA, auto WS) {
            hipLaunchKernelGGL((k_score_counts_pixel<decltype(WP)::value, decltype(WA)::value, decltype(WS)::value>), grid,
                               dim3(64 * QT_WAVES), 0, s, g);
        });
        HIP_TRY(hipGetLastError());
        return CAE_OK;
    }
    HIP_TRY(hipMemsetAsync(count, 0, (size_t)n_level * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(n, 0, sizeof(int64_t), s));
    const dim3 grid((unsigned)quantile_pool_groups(g.total));
    with_widths(P, A, S, [&](auto WP, auto WA, auto WS) {
        hipLaunchKernelGGL((k_score_counts_pool<decltype(WP)::value, decltype(WA)::value, decltype(WS)::value>), grid, dim3(256), 0, s,
                           g);
    });
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_interval_bounds(const void* pred, int pred_kind, int64_t pred_stride, const void* scale, int scale_kind, int64_t scale_stride,
                        int64_t n_case, int64_t plane, const double* q, int group, double* lower, double* upper, void* hip_stream) {
    const CaseOperand P{pred, pred_kind, pred_stride}, S{scale, scale ? scale_kind : CAE_ELEM_F32, scale ? scale_stride : 0};
    if (!known(P) || !known(S) || !quantile_sizes_ok(n_case, plane, group))
        return fail(CAE_ERR_ARG, "cae_interval_bounds: bad argument (CAE_ELEM_* kinds, 0 <= n_case < 2^31, plane >= 0, at most 2^40 "
                                 "pixels, group 0 or 1)");
    if (P.stride < 0 || S.stride < 0) return fail(CAE_ERR_ARG, "cae_interval_bounds: negative stride");
    if (n_case == 0 || plane == 0) return CAE_OK;
    if (!P.p || !q || !lower || !upper) return fail(CAE_ERR_ARG, "cae_interval_bounds: null pointer");
    if (shorter(P, plane) || (S.p && shorter(S, plane))) return fail(CAE_ERR_ARG, "cae_interval_bounds: a case stride is shorter than the plane");
    if (reaches(P, n_case, plane) || (S.p && reaches(S, n_case, plane)))
        return fail(CAE_ERR_ARG, "cae_interval_bounds: an operand reaches 2^60 elements from its pointer");
    if (misaligned(P) || (S.p && misaligned(S)) || ((uintptr_t)q & 7) || ((uintptr_t)lower & 7) || ((uintptr_t)upper & 7))
        return fail(CAE_ERR_ARG, "cae_interval_bounds: pointers must be aligned to their element size");
    QbArgs b;
    memset(&b, 0, sizeof b);
    b.p = (const unsigned char*)P.p, b.s = (const unsigned char*)S.p, b.p_stride = P.stride, b.s_stride = S.p ? S.stride : 0;
    b.n_case = n_case, b.plane = plane, b.total = n_case * plane, b.p_be = P.kind & 1, b.s_be = S.p ? S.kind & 1 : 0, b.pooled = group;
    b.q = q, b.lower = lower, b.upper = upper;
    const dim3 grid((unsigned)ceil_capped(b.total, 256 * 4, 8192));
    with_widths(P, P, S, [&](auto WP, auto, auto WS) {
        hipLaunchKernelGGL((k_interval_bounds<decltype(WP)::value, decltype(WS)::value>), grid, dim3(256), 0, (hipStream_t)hip_stream, b);
    });
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

// ---- novelty: K nearest neighbours between two sets of rows -------------------------------------------------------------

// Runs of reference tiles, one per workgroup of a query tile: about NB_RESIDENT workgroups in all where the call is large
// enough - two rounds of what the device holds at once, two workgroups on each of its 256 CUs by k_nb_tile's registers.  The
// order of the candidates is total, so the cut changes no result.
constexpr int64_t NB_RESIDENT = 1024;

static int64_t neighbours_tiles_per_split(int64_t n_query, int64_t n_ref) {
    const int64_t q_tiles = (n_query + NB_T - 1) / NB_T, r_tiles = (n_ref + NB_T - 1) / NB_T;
    int64_t want = (NB_RESIDENT + q_tiles - 1) / q_tiles;
    if (want > r_tiles) want = r_tiles;
    if (want > 65535) want = 65535;
    if (want < 1) want = 1;
    return (r_tiles + want - 1) / want;
}

static int64_t neighbours_splits(int64_t n_query, int64_t n_ref) {
    if (n_ref < 1) return 0;
    const int64_t per = neighbours_tiles_per_split(n_query, n_ref);
    return ((n_ref + NB_T - 1) / NB_T + per - 1) / per;
}

static bool neighbours_sizes_ok(int64_t n_query, int64_t n_ref, int k) {
    return n_query >= 0 && n_query <= 0x7fffffffLL && n_ref >= 0 && n_ref <= 0x7fffffffLL && k >= 1 && k <= NB_MAX_K;
}

// the workspace: the splits' partial lists, distances then indices, then the validity of the queries and of the references
static int64_t neighbours_part_entries(int64_t n_query, int64_t n_ref, int k) { return neighbours_splits(n_query, n_ref) * n_query * k; }

int64_t cae_case_neighbours_workspace_bytes(int64_t n_query, int64_t n_ref, int k) {
    if (n_query < 1 || !neighbours_sizes_ok(n_query, n_ref, k)) return 0;
    const int64_t e = neighbours_part_entries(n_query, n_ref, k);
    return e * 8 + (e + 1) / 2 * 8 + (n_query + n_ref + 1) / 2 * 8;
}

int cae_case_neighbours(const float* query, int64_t n_query, int64_t query_stride, const float* ref, int64_t n_ref, int64_t ref_stride,
                        int64_t dim, int k, int64_t ref_base, int64_t self_offset, int merge, double* dist2, int32_t* index,
                        int32_t* count, void* workspace, int64_t workspace_bytes, void* hip_stream) {
    if (!neighbours_sizes_ok(n_query, n_ref, k) || ref_base < 0 || ref_base + n_ref > 0x7fffffffLL || self_offset < -1 ||
        (merge != 0 && merge != 1))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: bad argument (0 <= n_query, n_ref < 2^31, 1 <= k <= %d, 0 <= ref_base, ref_base + "
                                 "n_ref < 2^31, self_offset >= -1, merge 0 or 1)", NB_MAX_K);
    if ((n_query > 0 || n_ref > 0) && dim < 1) return fail(CAE_ERR_ARG, "cae_case_neighbours: dim must be at least 1 while rows exist");
    const CaseOperand Q{query, CAE_ELEM_F32, query_stride}, R{ref, CAE_ELEM_F32, ref_stride};
    if ((n_query > 0 && shorter(Q, dim)) || (n_ref > 0 && shorter(R, dim)))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: a row stride is shorter than dim");
    if (!dist2 || !index || !count) return fail(CAE_ERR_ARG, "cae_case_neighbours: null output");
    if ((n_query > 0 && !Q.p) || (n_query > 0 && n_ref > 0 && !R.p)) return fail(CAE_ERR_ARG, "cae_case_neighbours: null operand with rows to read");
    if ((n_query > 0 && reaches(Q, n_query, dim)) || (n_ref > 0 && reaches(R, n_ref, dim)))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: an operand reaches 2^60 elements from its pointer");
    if (misaligned(Q) || misaligned(R) || ((uintptr_t)dist2 & 7) || ((uintptr_t)index & 3) || ((uintptr_t)count & 3))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: pointers must be aligned to their element size");
    if (n_query == 0) return CAE_OK;
    const int64_t need = cae_case_neighbours_workspace_bytes(n_query, n_ref, k);
    if (workspace_short(workspace, workspace_bytes, need))
        return fail(CAE_ERR_ARG, "cae_case_neighbours: needs a workspace of %lld bytes (cae_case_neighbours_workspace_bytes)",
                    (long long)need);
    if (n_ref == 0 && merge == 1) return CAE_OK;        // nothing joins the lists
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t entries = neighbours_part_entries(n_query, n_ref, k);
    NbArgs a;
    memset(&a, 0, sizeof a);
    a.q = query, a.r = ref, a.n_q = n_query, a.q_stride = query_stride, a.n_r = n_ref, a.r_stride = ref_stride, a.dim = dim;
    a.ref_base = ref_base, a.self_offset = self_offset, a.k = k, a.merge = merge;
    a.n_split = (int)neighbours_splits(n_query, n_ref);
    a.tiles_per_split = n_ref > 0 ? (int)neighbours_tiles_per_split(n_query, n_ref) : 0;
    a.part_d = (unsigned long long*)workspace;
    a.part_i = (int*)(a.part_d + entries);
    int* ok = a.part_i + (entries + 1) / 2 * 2;
    a.q_ok = ok, a.r_ok = ok + n_query;
    a.dist2 = dist2, a.index = (int*)index, a.count = (int*)count;
    hipLaunchKernelGGL((k_nb_valid<256>), dim3((unsigned)ceil_capped(n_query, 4, 8192)), dim3(256), 0, s, query, (long long)n_query,
                       (long long)query_stride, (long long)dim, ok);
    HIP_TRY(hipGetLastError());
    if (n_ref > 0) {
        hipLaunchKernelGGL((k_nb_valid<256>), dim3((unsigned)ceil_capped(n_ref, 4, 8192)), dim3(256), 0, s, ref, (long long)n_ref,
                           (long long)ref_stride, (long long)dim, ok + n_query);
        HIP_TRY(hipGetLastError());
        const dim3 grid((unsigned)((n_query + NB_T - 1) / NB_T), (unsigned)a.n_split);
        const size_t lds = (size_t)NB_TILE_BYTES + (size_t)k * NB_T * (sizeof(unsigned long long) + sizeof(int));      // at most 57 856 bytes
        hipLaunchKernelGGL((k_nb_tile<256>), grid, dim3(256), lds, s, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((k_nb_merge<NB_T>), dim3((unsigned)((n_query + NB_T - 1) / NB_T)), dim3(NB_T), 0, s, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

}  // extern "C"
