// host_fss.h - host only: neighbourhood skill, the window sums of the Fractions Skill Score: cae_case_fss over kernels_fss.h.
// Included by stateless_host.h alone.
#pragma once

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
        if (!is_finite(thresholds[t])) return fail(CAE_ERR_ARG, "cae_case_fss: the thresholds must be finite");
    for (int t = 0; t < n_thr; t++)
        if (sides[t] != 0 && sides[t] != 1) return fail(CAE_ERR_ARG, "cae_case_fss: a side must be 0 (above) or 1 (below)");
    for (int j = 0; j < n_width; j++)
        if (widths[j] < 1 || widths[j] > FS_MAX_N || widths[j] % 2 == 0 || (j > 0 && widths[j] <= widths[j - 1]))
            return fail(CAE_ERR_ARG, "cae_case_fss: the widths must be odd, from 1 to %d and strictly ascending", FS_MAX_N);
    const int64_t plane = h * w;
    if (any_shorter({{P, plane}, {A, plane}})) return fail(CAE_ERR_ARG, "cae_case_fss: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{P, plane}, {A, plane}}))
        return fail(CAE_ERR_ARG, "cae_case_fss: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({P, A})) return fail(CAE_ERR_ARG, "cae_case_fss: pointers must be aligned to their element size");
    const int64_t need = cae_case_fss_workspace_bytes(n_case, h, w, n_thr);
    if (workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_case_fss", need);
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
    with_kinds(P.kind, A.kind, [&](auto KP, auto KA) {
        hipLaunchKernelGGL((k_fss_bits<decltype(KP)::value, decltype(KA)::value>), grid_b, dim3(64 * FS_WAVES), 0, s, b);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_fss_windows<FS_WAVES>), dim3((unsigned)ceil_capped(g.items, FS_WAVES, FS_WIN_GROUPS)), dim3(64 * FS_WAVES), 0,
                       s, (const unsigned long long*)workspace, (unsigned long long*)sums, g);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
