// host_case_pages.h - host only: the case pages' value range and rendered images, cae_case_range and cae_render_cases, over
// kernels_stateless.h.  Included by stateless_host.h alone.
#pragma once

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
    if (any_shorter({{S, plane}, {B, plane}})) return fail(CAE_ERR_ARG, "%s: a case stride is shorter than the plane", who);
    if (any_misaligned({S, B})) return fail(CAE_ERR_ARG, "%s: pointers must be aligned to their element size", who);
    return CAE_OK;
}

int cae_case_range(const void* src, int src_kind, int64_t src_stride, const void* sub, int sub_kind, int64_t sub_stride,
                   int64_t n_case, int64_t plane, double* out, void* workspace, int64_t workspace_bytes,
                   void* hip_stream) {
    if (!out || ((uintptr_t)out & 7) || n_case < 1 || plane < 1) return fail(CAE_ERR_ARG, "cae_case_range: bad argument");
    const CaseOperand S{src, src_kind, src_stride}, B{sub, sub_kind, sub_stride};
    if (const int rc = case_pair_check("cae_case_range", S, B, plane)) return rc;
    const int64_t nch = case_chunks(plane);
    if (nch > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_case_range: plane too large");
    const int64_t need = cae_case_range_workspace_bytes(n_case, plane);
    if (workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_case_range", need);
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
    if (!is_finite(lo) || !is_finite(hi) || !is_finite(hi - lo))
        return fail(CAE_ERR_ARG, "cae_render_cases: lo, hi and hi - lo must be finite");
    const CaseOperand S{src, src_kind, src_stride}, B{sub, sub_kind, sub_stride};
    if (const int rc = case_pair_check("cae_render_cases", S, B, height * width)) return rc;
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
