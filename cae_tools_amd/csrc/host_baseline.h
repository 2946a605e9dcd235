// host_baseline.h - host only: skill against interpolating the input, cae_case_baseline, over kernels_baseline.h.
// Included by stateless_host.h alone.
#pragma once

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
    if (any_shorter({{L, plane_in}, {A, plane}, {P, plane}}))
        return fail(CAE_ERR_ARG, "cae_case_baseline: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{L, plane_in}, {A, plane}, {P, plane}}) || (field && (__int128)n_case * plane > ((__int128)1 << 60)))
        return fail(CAE_ERR_ARG, "cae_case_baseline: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({L, A, P}) || ((uintptr_t)sums & 7) || ((uintptr_t)field & 7) || ((uintptr_t)workspace & 7))
        return fail(CAE_ERR_ARG, "cae_case_baseline: pointers must be aligned to their element size, the workspace to 8 bytes");
    const int64_t need = cae_case_baseline_workspace_bytes(n_case, h_out, w_out);
    if (!workspace || workspace_bytes < need) return no_workspace("cae_case_baseline", need);
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
    // the widths of a, then of p: <mode, 4, 4>, <mode, 4, 8>, <mode, 8, 4>, <mode, 8, 8> are instantiated in this order
    auto launch = [&](auto MODE) {
        with_widths(A, P.p ? P : A, CaseOperand{}, [&](auto WA, auto WP, auto) {
            hipLaunchKernelGGL((k_case_baseline<decltype(MODE)::value, decltype(WA)::value, decltype(WP)::value>), grid, dim3(256), 0, s, a);
        });
    };
    switch (mode) {
    case CAE_INTERP_NEAREST: launch(std::integral_constant<int, 0>()); break;
    case CAE_INTERP_BILINEAR: launch(std::integral_constant<int, 1>()); break;
    default: launch(std::integral_constant<int, 2>()); break;
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_baseline_fold, dim3((unsigned)ceil_capped(n_case * BL_SUMS, 256, 4096)), dim3(256), 0, s,
                       (const double*)workspace, (long long)n_case, (int)baseline_items(h_out, w_out), sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
