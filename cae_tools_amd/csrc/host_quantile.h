// host_quantile.h - host only: prediction intervals, exact order statistics of the absolute residual, the counts below them and the
// bounds: cae_score_quantiles, cae_score_counts, cae_interval_bounds over kernels_quantile.h.  Included by stateless_host.h alone.
#pragma once

static bool quantile_sizes_ok(int64_t n_case, int64_t plane, int group) {
    return n_case >= 0 && n_case <= 0x7fffffffLL && plane >= 0 && plane <= ((int64_t)1 << 40) &&
           (__int128)n_case * plane <= ((__int128)1 << 40) && (group == 0 || group == 1);
}

// The operand rungs cae_score_quantiles and cae_score_counts share, after the sizes; S is the optional scale.
static int quantile_operand_check(const char* who, const CaseOperand& P, const CaseOperand& A, const CaseOperand& S, int64_t n_case,
                                  int64_t plane) {
    if (!P.p || !A.p) return fail(CAE_ERR_ARG, "%s: null pointer", who);
    if (any_shorter({{P, plane}, {A, plane}, {S, plane}})) return fail(CAE_ERR_ARG, "%s: a case stride is shorter than the plane", who);
    if (any_reaches(n_case, {{P, plane}, {A, plane}, {S, plane}}))
        return fail(CAE_ERR_ARG, "%s: an operand reaches 2^60 elements from its pointer", who);
    if (any_misaligned({P, A, S})) return fail(CAE_ERR_ARG, "%s: pointers must be aligned to their element size", who);
    return CAE_OK;
}

static void quantile_args(QtArgs& g, const CaseOperand& P, const CaseOperand& A, const CaseOperand& S, int64_t n_case, int64_t plane,
                          int n_level) {
    memset(&g, 0, sizeof g);
    g.p = (const unsigned char*)P.p, g.a = (const unsigned char*)A.p, g.s = (const unsigned char*)S.p;
    g.p_stride = P.stride, g.a_stride = A.stride, g.s_stride = S.stride;
    g.p_be = P.kind & 1, g.a_be = A.kind & 1, g.s_be = S.kind & 1;
    g.n_level = n_level, g.n_case = n_case, g.plane = plane;
    g.n_tile = (plane + 63) / 64, g.total = n_case * plane;
}

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
        S = optional_operand(scale, scale_kind, scale_stride);
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
    if (need > 0 && workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_score_quantiles", need);
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
        S = optional_operand(scale, scale_kind, scale_stride);
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
    const CaseOperand P{pred, pred_kind, pred_stride}, S = optional_operand(scale, scale_kind, scale_stride);
    if (!known(P) || !known(S) || !quantile_sizes_ok(n_case, plane, group))
        return fail(CAE_ERR_ARG, "cae_interval_bounds: bad argument (CAE_ELEM_* kinds, 0 <= n_case < 2^31, plane >= 0, at most 2^40 "
                                 "pixels, group 0 or 1)");
    if (P.stride < 0 || S.stride < 0) return fail(CAE_ERR_ARG, "cae_interval_bounds: negative stride");
    if (n_case == 0 || plane == 0) return CAE_OK;
    if (!P.p || !q || !lower || !upper) return fail(CAE_ERR_ARG, "cae_interval_bounds: null pointer");
    if (any_shorter({{P, plane}, {S, plane}})) return fail(CAE_ERR_ARG, "cae_interval_bounds: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{P, plane}, {S, plane}}))
        return fail(CAE_ERR_ARG, "cae_interval_bounds: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({P, S}) || ((uintptr_t)q & 7) || ((uintptr_t)lower & 7) || ((uintptr_t)upper & 7))
        return fail(CAE_ERR_ARG, "cae_interval_bounds: pointers must be aligned to their element size");
    QbArgs b;
    memset(&b, 0, sizeof b);
    b.p = (const unsigned char*)P.p, b.s = (const unsigned char*)S.p, b.p_stride = P.stride, b.s_stride = S.stride;
    b.n_case = n_case, b.plane = plane, b.total = n_case * plane, b.p_be = P.kind & 1, b.s_be = S.kind & 1, b.pooled = group;
    b.q = q, b.lower = lower, b.upper = upper;
    const dim3 grid((unsigned)ceil_capped(b.total, 256 * 4, 8192));
    with_widths(P, P, S, [&](auto WP, auto, auto WS) {
        hipLaunchKernelGGL((k_interval_bounds<decltype(WP)::value, decltype(WS)::value>), grid, dim3(256), 0, (hipStream_t)hip_stream, b);
    });
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
