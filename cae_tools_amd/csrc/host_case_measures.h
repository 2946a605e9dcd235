// host_case_measures.h - host only: the evaluator's per-case sums, cae_case_measures, over kernels_stateless.h.  case_chunks, its cut
// of a plane, is also the case pages' and the value distributions'.  Included by stateless_host.h alone.
#pragma once

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
    if (any_shorter({{P, plane}, {A, plane}}))
        return fail(CAE_ERR_ARG, "cae_case_measures: a case stride is shorter than the plane");
    if (any_misaligned({P, A}) || ((uintptr_t)out & 7))
        return fail(CAE_ERR_ARG, "cae_case_measures: pointers must be aligned to their element size");
    const int64_t nch = case_chunks(plane);
    if (nch > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_case_measures: plane too large");
    const int64_t need = cae_case_measures_workspace_bytes(n_case, plane);
    if (need > 0 && workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_case_measures", need);
    hipStream_t s = (hipStream_t)hip_stream;
    const int64_t items = n_case * nch;
    double* dst = nch > 1 ? (double*)workspace : out;
    const dim3 grid((unsigned)ceil_capped(items, CM_WAVES, 8192));
    with_kinds(P.kind, A.kind, [&](auto KP, auto KA) {
        hipLaunchKernelGGL((k_case_measures<decltype(KP)::value, decltype(KA)::value>), grid, dim3(256), 0, s,
                           (const unsigned char*)P.p, (long long)P.stride, (const unsigned char*)A.p, (long long)A.stride,
                           (long long)plane, (int)nch, (long long)items, dst);
    });
    HIP_TRY(hipGetLastError());
    if (nch > 1) {
        hipLaunchKernelGGL(k_case_fold, dim3((unsigned)ceil_capped(n_case, 256, 4096)), dim3(256), 0, s,
                           (const double*)workspace, (long long)n_case, (int)nch, out);
        HIP_TRY(hipGetLastError());
    }
    return CAE_OK;
}
