// host_blend.h - host only: the error moments a weighted blend of models is fitted from, and the blended field:
// cae_case_error_moments and cae_blend_predictions over kernels_blend.h.  Included by stateless_host.h alone.
#pragma once

// so many workgroups at the most; a wave takes one work item at a time and strides over the rest
constexpr int64_t BD_MOMENT_GROUPS = 4096;
// likewise for the blended field: a lane takes four elements at a time
constexpr int64_t BD_FIELD_GROUPS = 2048;

static int moments_width(int n_pred) { return 1 + n_pred + n_pred * (n_pred + 1) / 2; }
static int moments_pitch(int n_pred) { return (moments_width(n_pred) + 1) & ~1; }

int64_t cae_case_error_moments_workspace_bytes(int64_t n_case, int64_t plane, int n_pred) {
    if (n_case < 1 || plane < 1 || n_pred < 1 || n_pred > CP_MAX || (__int128)n_case * plane > ((__int128)1 << 60)) return 0;
    return n_case * compare_tiles(plane) * moments_pitch(n_pred) * (int64_t)sizeof(double);
}

int cae_case_error_moments(const void* const* pred_ptrs, int pred_kind, const int64_t* pred_case_strides, int n_pred, const void* actual,
                           int actual_kind, int64_t actual_case_stride, int64_t n_case, int64_t plane, double* sums, void* workspace,
                           int64_t workspace_bytes, void* hip_stream) {
    const CaseOperand A{actual, actual_kind, actual_case_stride};
    if (!kind_known(pred_kind) || !known(A) || n_pred < 1 || n_pred > CP_MAX || n_case < 0 || plane < 0)
        return fail(CAE_ERR_ARG, "cae_case_error_moments: bad argument (CAE_ELEM_* kinds, 1 <= n_pred <= %d, n_case >= 0, plane >= 0)", CP_MAX);
    if (!pred_ptrs || !pred_case_strides) return fail(CAE_ERR_ARG, "cae_case_error_moments: null list of predictions");
    CaseOperand P[CP_MAX];
    for (int m = 0; m < n_pred; m++) P[m] = CaseOperand{pred_ptrs[m], pred_kind, pred_case_strides[m]};
    if (A.stride < 0 || std::any_of(P, P + n_pred, [](const CaseOperand& o) { return o.stride < 0; }))
        return fail(CAE_ERR_ARG, "cae_case_error_moments: negative stride");
    if (n_case == 0 || plane == 0) return CAE_OK;
    if (!A.p || !sums || std::any_of(P, P + n_pred, [](const CaseOperand& o) { return !o.p; }))
        return fail(CAE_ERR_ARG, "cae_case_error_moments: null pointer");
    bool is_shorter = any_shorter({{A, plane}}), does_reach = any_reaches(n_case, {{A, plane}}), is_misaligned = any_misaligned({A});
    for (int m = 0; m < n_pred; m++) {
        is_shorter = is_shorter || any_shorter({{P[m], plane}});
        does_reach = does_reach || any_reaches(n_case, {{P[m], plane}});
        is_misaligned = is_misaligned || any_misaligned({P[m]});
    }
    if (is_shorter) return fail(CAE_ERR_ARG, "cae_case_error_moments: a case stride is shorter than the plane");
    if (does_reach || (__int128)n_case * plane > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_case_error_moments: an operand reaches 2^60 elements from its pointer");
    if (is_misaligned || ((uintptr_t)sums & 7) || ((uintptr_t)workspace & 15))
        return fail(CAE_ERR_ARG, "cae_case_error_moments: pointers must be aligned to their element size, the workspace to 16 bytes");
    const int64_t need = cae_case_error_moments_workspace_bytes(n_case, plane, n_pred);
    if (!workspace || workspace_bytes < need) return no_workspace("cae_case_error_moments", need);
    hipStream_t s = (hipStream_t)hip_stream;
    BdMoments a;
    memset(&a, 0, sizeof a);
    for (int m = 0; m < n_pred; m++) a.p[m] = (const unsigned char*)P[m].p, a.p_stride[m] = P[m].stride;
    a.a = (const unsigned char*)A.p, a.a_stride = A.stride;
    a.n_case = n_case, a.plane = plane, a.n_tile = compare_tiles(plane);
    a.items = a.n_tile * ((n_case + CP_RUN - 1) / CP_RUN);
    a.n_pred = n_pred, a.width = moments_width(n_pred), a.pitch = moments_pitch(n_pred), a.part = (double*)workspace;
    const int64_t groups = (a.items + CP_WAVES - 1) / CP_WAVES, fold_groups = (n_case + CP_WAVES - 1) / CP_WAVES;
    const dim3 grid((unsigned)(groups < BD_MOMENT_GROUPS ? groups : BD_MOMENT_GROUPS)), block(64 * CP_WAVES);
    const dim3 fold_grid((unsigned)(fold_groups < BD_MOMENT_GROUPS ? fold_groups : BD_MOMENT_GROUPS));
    // the loops are unrolled for 2, 4 or 8 predictions: the smallest that holds n_pred
    auto launch = [&](auto MM) {
        with_kinds(pred_kind, A.kind, [&](auto KP, auto KA) {
            hipLaunchKernelGGL((k_case_error_moments<decltype(KP)::value, decltype(KA)::value, decltype(MM)::value>), grid, block, 0, s, a);
        });
        hipLaunchKernelGGL((k_moments_fold<decltype(MM)::value>), fold_grid, block, 0, s, (const double*)workspace, (long long)n_case,
                           (long long)a.n_tile, a.width, a.pitch, sums);
    };
    if (n_pred <= 2) launch(std::integral_constant<int, 2>());
    else if (n_pred <= 4) launch(std::integral_constant<int, 4>());
    else launch(std::integral_constant<int, 8>());
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_blend_predictions(const void* const* pred_ptrs, int pred_kind, const int64_t* pred_case_strides, int n_pred, const double* weights,
                          double intercept, int64_t n_case, int64_t case_elems, double* out, int64_t out_case_stride, void* hip_stream) {
    if (!kind_known(pred_kind) || n_pred < 1 || n_pred > CP_MAX || n_case < 0 || case_elems < 0)
        return fail(CAE_ERR_ARG, "cae_blend_predictions: bad argument (a CAE_ELEM_* kind, 1 <= n_pred <= %d, n_case >= 0, case_elems >= 0)", CP_MAX);
    if (!pred_ptrs || !pred_case_strides || !weights) return fail(CAE_ERR_ARG, "cae_blend_predictions: null list of predictions or weights");
    CaseOperand P[CP_MAX];
    for (int m = 0; m < n_pred; m++) P[m] = CaseOperand{pred_ptrs[m], pred_kind, pred_case_strides[m]};
    if (out_case_stride < 0 || std::any_of(P, P + n_pred, [](const CaseOperand& o) { return o.stride < 0; }))
        return fail(CAE_ERR_ARG, "cae_blend_predictions: negative stride");
    if (!is_finite(intercept) || !std::all_of(weights, weights + n_pred, is_finite))
        return fail(CAE_ERR_ARG, "cae_blend_predictions: the weights and the intercept must be finite");
    if (n_case == 0 || case_elems == 0) return CAE_OK;
    if (!out || std::any_of(P, P + n_pred, [](const CaseOperand& o) { return !o.p; }))
        return fail(CAE_ERR_ARG, "cae_blend_predictions: null pointer");
    const CaseOperand O{out, CAE_ELEM_F64, out_case_stride};
    bool is_shorter = any_shorter({{O, case_elems}}), does_reach = any_reaches(n_case, {{O, case_elems}}), is_misaligned = any_misaligned({O});
    for (int m = 0; m < n_pred; m++) {
        is_shorter = is_shorter || any_shorter({{P[m], case_elems}});
        does_reach = does_reach || any_reaches(n_case, {{P[m], case_elems}});
        is_misaligned = is_misaligned || any_misaligned({P[m]});
    }
    if (is_shorter) return fail(CAE_ERR_ARG, "cae_blend_predictions: a case stride is shorter than the case");
    if (does_reach || (__int128)n_case * case_elems > ((__int128)1 << 60))
        return fail(CAE_ERR_ARG, "cae_blend_predictions: an operand reaches 2^60 elements from its pointer");
    if (is_misaligned) return fail(CAE_ERR_ARG, "cae_blend_predictions: pointers must be aligned to their element size");
    BdField a;
    memset(&a, 0, sizeof a);
    // a candidate whose weight is exactly 0 is not read; the others keep their order.  16-byte accesses where the output
    // and every kept candidate start on a 16-byte boundary in every case
    const int64_t line = 16 / elem_bytes(pred_kind);
    a.vec = !((uintptr_t)out & 15) && out_case_stride % 2 == 0;
    for (int m = 0; m < n_pred; m++) {
        if (weights[m] == 0.0) continue;
        a.p[a.n_kept] = (const unsigned char*)P[m].p, a.p_stride[a.n_kept] = P[m].stride, a.w[a.n_kept] = weights[m];
        a.vec = a.vec && !((uintptr_t)P[m].p & 15) && P[m].stride % line == 0;
        a.n_kept++;
    }
    a.c = intercept, a.per = case_elems, a.n_quad = (case_elems + BD_VEC - 1) / BD_VEC, a.items = n_case * a.n_quad;
    a.out = out, a.out_stride = out_case_stride;
    const int64_t groups = (a.items + BD_THREADS - 1) / BD_THREADS;
    const dim3 grid((unsigned)(groups < BD_FIELD_GROUPS ? groups : BD_FIELD_GROUPS)), block(BD_THREADS);
    auto launch = [&](auto MM) {
        with_kind(pred_kind, [&](auto KP) {
            hipLaunchKernelGGL((k_blend_predictions<decltype(KP)::value, decltype(MM)::value>), grid, block, 0, (hipStream_t)hip_stream, a);
        });
    };
    if (a.n_kept <= 2) launch(std::integral_constant<int, 2>());
    else if (a.n_kept <= 4) launch(std::integral_constant<int, 4>());
    else launch(std::integral_constant<int, 8>());
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
