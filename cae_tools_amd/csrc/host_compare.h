// host_compare.h - host only: models compared on the same pixels and the bootstrap of a per-case table of sums:
// cae_case_compare and cae_bootstrap_sums over kernels_compare.h.  Included by stateless_host.h alone.
#pragma once

static int64_t compare_tiles(int64_t plane) { return (plane + CP_TILE - 1) / CP_TILE; }

int64_t cae_case_compare_workspace_bytes(int64_t n_case, int64_t plane, int n_pred) {
    if (n_case < 1 || plane < 1 || n_pred < 1 || n_pred > CP_MAX || (__int128)n_case * plane > ((__int128)1 << 60)) return 0;
    return n_case * compare_tiles(plane) * (2 + 4 * n_pred) * (int64_t)sizeof(double);
}

int cae_case_compare(const void* const* pred_ptrs, int pred_kind, const int64_t* pred_case_strides, int n_pred, const void* actual,
                     int actual_kind, int64_t actual_case_stride, int64_t n_case, int64_t plane, double* sums, void* workspace,
                     int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand A{actual, actual_kind, actual_case_stride};
    if (!kind_known(pred_kind) || !known(A) || n_pred < 1 || n_pred > CP_MAX || n_case < 0 || plane < 0)
        return fail(CAE_ERR_ARG, "cae_case_compare: bad argument (CAE_ELEM_* kinds, 1 <= n_pred <= %d, n_case >= 0, plane >= 0)", CP_MAX);
    if (!pred_ptrs || !pred_case_strides) return fail(CAE_ERR_ARG, "cae_case_compare: null list of predictions");
    CaseOperand P[CP_MAX];
    for (int m = 0; m < n_pred; m++) P[m] = CaseOperand{pred_ptrs[m], pred_kind, pred_case_strides[m]};
    if (A.stride < 0 || std::any_of(P, P + n_pred, [](const CaseOperand& o) { return o.stride < 0; }))
        return fail(CAE_ERR_ARG, "cae_case_compare: negative stride");
    if (n_case == 0 || plane == 0) return CAE_OK;
    if (!A.p || !sums || std::any_of(P, P + n_pred, [](const CaseOperand& o) { return !o.p; }))
        return fail(CAE_ERR_ARG, "cae_case_compare: null pointer");
    bool is_shorter = any_shorter({{A, plane}}), does_reach = any_reaches(n_case, {{A, plane}}), is_misaligned = any_misaligned({A});
    for (int m = 0; m < n_pred; m++) {
        is_shorter = is_shorter || any_shorter({{P[m], plane}});
        does_reach = does_reach || any_reaches(n_case, {{P[m], plane}});
        is_misaligned = is_misaligned || any_misaligned({P[m]});
    }
    if (is_shorter) return fail(CAE_ERR_ARG, "cae_case_compare: a case stride is shorter than the plane");
    if (does_reach || (__int128)n_case * plane > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_case_compare: an operand reaches 2^60 elements from its pointer");
    if (is_misaligned || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 15))
        return fail(CAE_ERR_ARG, "cae_case_compare: pointers must be aligned to their element size, the workspace to 16 bytes");
    const int64_t need = cae_case_compare_workspace_bytes(n_case, plane, n_pred);
    if (!workspace || workspace_bytes < need) return no_workspace("cae_case_compare", need);
    hipStream_t s = (hipStream_t)hip_stream;
    CpArgs a;
    memset(&a, 0, sizeof a);
    for (int m = 0; m < n_pred; m++) a.p[m] = (const unsigned char*)P[m].p, a.p_stride[m] = P[m].stride;
    a.a = (const unsigned char*)A.p, a.a_stride = A.stride;
    a.n_case = n_case, a.plane = plane, a.n_tile = compare_tiles(plane);
    a.items = a.n_tile * ((n_case + CP_RUN - 1) / CP_RUN);
    a.n_pred = n_pred, a.width = 2 + 4 * n_pred, a.part = (double*)workspace;
    const dim3 grid((unsigned)ceil_capped(a.items, CP_WAVES, 16384)), block(64 * CP_WAVES);
    const dim3 fold_grid((unsigned)ceil_capped(n_case, CP_WAVES, 8192));
    // the loops are unrolled for 2, 4 or 8 predictions: the smallest that holds n_pred
    auto launch = [&](auto MM) {
        with_kinds(pred_kind, A.kind, [&](auto KP, auto KA) {
            hipLaunchKernelGGL((k_case_compare<decltype(KP)::value, decltype(KA)::value, decltype(MM)::value>), grid, block, 0, s, a);
        });
        hipLaunchKernelGGL((k_compare_fold<decltype(MM)::value>), fold_grid, block, 0, s, (const double*)workspace, (long long)n_case,
                           (long long)a.n_tile, a.width, sums);
    };
    if (n_pred <= 2) launch(std::integral_constant<int, 2>());
    else if (n_pred <= 4) launch(std::integral_constant<int, 4>());
    else launch(std::integral_constant<int, 8>());
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_bootstrap_sums(const double* table, int64_t n_unit, int n_col, int64_t first_resample, int64_t n_resample, uint64_t seed,
                       double* out, void* hip_stream) {
    if (n_unit < 1 || n_unit > BS_MAX_UNIT || n_col < 1 || n_col > BS_MAX_COL || first_resample < 0 || n_resample < 0 ||
        first_resample > ((int64_t)1 << 32) || n_resample > ((int64_t)1 << 32) || first_resample + n_resample > ((int64_t)1 << 32))
        return fail(CAE_ERR_ARG, "cae_bootstrap_sums: bad argument (1 <= n_unit <= 2^20, 1 <= n_col <= %d, first_resample >= 0, "
                                 "n_resample >= 0, first_resample + n_resample <= 2^32)", BS_MAX_COL);
    if (n_resample == 0) return CAE_OK;
    if (!table || !out) return fail(CAE_ERR_ARG, "cae_bootstrap_sums: null pointer");
    if (((uintptr_t)table & 7) || ((uintptr_t)out & 7)) return fail(CAE_ERR_ARG, "cae_bootstrap_sums: pointers must be 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    BsArgs a;
    memset(&a, 0, sizeof a);
    a.table = table, a.out = out, a.seed = seed, a.first = first_resample, a.n_resample = n_resample;
    a.n_unit = (int)n_unit, a.n_col = n_col;
    const bool wide = n_resample * ((n_col + 3) / 4) >= BS_WIDE_ITEMS;
    a.n_group = wide ? (n_col + 3) / 4 : n_col;
    a.items = n_resample * a.n_group;
    const size_t bytes = (size_t)n_unit * n_col * sizeof(double);
    const bool lds = bytes <= (size_t)BS_LDS_BYTES;
    // staged: every workgroup copies the table first, so no more workgroups than keep the device busy share the resamples
    const dim3 grid((unsigned)ceil_capped(a.items, BS_THREADS, lds ? 2048 : 16384)), block(BS_THREADS);
    if (lds && wide) launch_with_lds<k_bootstrap_sums<4, true>>(grid, block, bytes, s, a);
    else if (lds) launch_with_lds<k_bootstrap_sums<1, true>>(grid, block, bytes, s, a);
    else if (wide) hipLaunchKernelGGL((k_bootstrap_sums<4, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_bootstrap_sums<1, false>), grid, block, 0, s, a);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
