// host_pixel_sums.h - host only: the per-pixel skill sums over the cases, cae_pixel_sums and cae_pixel_sums_about, over
// kernels_stateless.h.  Included by stateless_host.h alone.
#pragma once

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
    if (n_case < 0 || plane < 0 || case_chunk < 0 || !known(P) || !known(A) || !is_finite(shift))
        return fail(CAE_ERR_ARG, "cae_pixel_sums: bad argument");
    if (plane == 0) return CAE_OK;
    if (!sums || ((uintptr_t)sums & 7)) return fail(CAE_ERR_ARG, "cae_pixel_sums: sums_dev must be an 8-byte aligned pointer");
    hipStream_t s = (hipStream_t)hip_stream;
    if (n_case == 0) {      // no case, no pair: nine planes of zeros
        HIP_TRY(hipMemsetAsync(sums, 0, (size_t)plane * PS_SUMS * sizeof(double), s));
        return CAE_OK;
    }
    if (!P.p || !A.p) return fail(CAE_ERR_ARG, "cae_pixel_sums: bad argument");
    if (any_shorter({{P, plane}, {A, plane}})) return fail(CAE_ERR_ARG, "cae_pixel_sums: a case stride is shorter than the plane");
    if (any_misaligned({P, A})) return fail(CAE_ERR_ARG, "cae_pixel_sums: pointers must be aligned to their element size");
    const int ep = elem_bytes(P.kind), ea = elem_bytes(A.kind);
    const int64_t chunk = pixel_chunk(n_case, plane, case_chunk);
    const int64_t n_chunk = (n_case + chunk - 1) / chunk;
    const int64_t need = cae_pixel_sums_workspace_bytes(n_case, plane, case_chunk);
    if (need > 0 && workspace_short(workspace, workspace_bytes, need)) return no_workspace("cae_pixel_sums", need);
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
    with_kinds(P.kind, A.kind, [&](auto KP, auto KA) {
        constexpr int kp = decltype(KP)::value, ka = decltype(KA)::value;
        if (a.shifts) hipLaunchKernelGGL((k_pixel_sums<kp, ka, true>), grid, dim3(64), 0, s, a);
        else hipLaunchKernelGGL((k_pixel_sums<kp, ka, false>), grid, dim3(64), 0, s, a);
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
