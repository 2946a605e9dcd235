// host_spectra.h - host only: power spectra of prediction against target, cae_case_spectra, over kernels_spectra.h.
// Included by stateless_host.h alone.
#pragma once

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
    if (any_shorter({{P, plane}, {A, plane}}))
        return fail(CAE_ERR_ARG, "cae_case_spectra: a case stride is shorter than the plane");
    if (any_reaches(n_case, {{P, plane}, {A, plane}}))
        return fail(CAE_ERR_ARG, "cae_case_spectra: an operand reaches 2^60 elements from its pointer");
    if (any_misaligned({P, A}) || ((uintptr_t)wy & 7) || ((uintptr_t)wx & 7) || ((uintptr_t)bin & 3) ||
        ((uintptr_t)sums & 7) || ((uintptr_t)counted & 3) || ((uintptr_t)workspace & 15))
        return fail(CAE_ERR_ARG, "cae_case_spectra: pointers must be aligned to their element size, the workspace to 16 bytes");
    const int64_t need = cae_case_spectra_workspace_bytes(n_case, h, w, n_bin);
    if (workspace_bytes < need) return no_workspace("cae_case_spectra", need);
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
    case 4: launch_with_lds<k_case_spectra<4>>(grid, dim3(SP_THREADS), lds, s, a); break;
    case 2: launch_with_lds<k_case_spectra<2>>(grid, dim3(SP_THREADS), lds, s, a); break;
    default: launch_with_lds<k_case_spectra<1>>(grid, dim3(SP_THREADS), lds, s, a); break;
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_spectra_fold, dim3((unsigned)ceil_capped(n_case * n_bin * 4, 256, 8192)), dim3(256), 0, s,
                       (const double*)a.part, (long long)n_case, (int)n_band, (int)n_bin, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
