// host_strata.h - host only: skill by stratum, the error sums conditioned on a third field: cae_strata_sums over
// kernels_strata.h.  Included by stateless_host.h alone.
#pragma once

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
        if (!is_finite(edges[j]) || (j > 0 && !(edges[j] > edges[j - 1])))
            return fail(CAE_ERR_ARG, "cae_strata_sums: the edges must be finite and strictly ascending");
    for (int k = 0; k < n_strata; k++)
        if (!is_finite(shift_a[k]) || !is_finite(shift_p[k]))
            return fail(CAE_ERR_ARG, "cae_strata_sums: the shifts must be finite");
    const int64_t plane = h * w, plane_s = sh * sw;
    if (any_shorter({{P, plane}, {A, plane}, {S, plane_s}}))
        return fail(CAE_ERR_ARG, "cae_strata_sums: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{P, plane}, {A, plane}, {S, plane_s}}))
        return fail(CAE_ERR_ARG, "cae_strata_sums: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({P, A, S})) return fail(CAE_ERR_ARG, "cae_strata_sums: pointers must be aligned to their element size");
    const int64_t need = cae_strata_sums_workspace_bytes(n_case, h, w, n_strata);
    if (workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_strata_sums", need);
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
    with_kinds(P.kind, A.kind, [&](auto KP, auto KA) {
        hipLaunchKernelGGL((k_strata_sums<decltype(KP)::value, decltype(KA)::value>), grid, dim3(64 * ST_WAVES), 0, s, a);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_strata_fold<ST_WAVES>), dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, (const double*)workspace,
                       (int)n_group, per, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
