// host_loader.h - host only: the loader's passes over a variable - scan, normalise and pack, invert a permutation,
// denormalise, metric sums, byte swap - over kernels_stateless.h.  Included by stateless_host.h alone, as every host_*.h.
#pragma once

int cae_scan_f32(const float* x, int64_t n, void* hip_stream, double* out3) {
    if (!x || n < 1 || !out3) return fail(CAE_ERR_ARG, "cae_scan_f32: bad argument");
    hipStream_t s = (hipStream_t)hip_stream;
    const int blocks = (int)ceil_capped(n, 256 * 16, 1024);
    double* part = nullptr;
    HIP_TRY(hipMalloc(&part, (size_t)blocks * 3 * sizeof(double)));
    hipLaunchKernelGGL(k_scan, dim3(blocks), dim3(256), 0, s, x, (long long)n, part);
    std::vector<double> host((size_t)blocks * 3);
    hipError_t ce = hipMemcpyAsync(host.data(), part, host.size() * sizeof(double), hipMemcpyDeviceToHost, s);
    if (ce == hipSuccess) ce = hipStreamSynchronize(s);
    (void)hipFree(part);
    if (ce != hipSuccess) return fail(CAE_ERR_HIP, "cae_scan_f32: %s", hipGetErrorString(ce));
    double cnt = 0, lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < blocks; i++) {
        cnt += host[3 * i];
        lo = std::fmin(lo, host[3 * i + 1]);
        hi = std::fmax(hi, host[3 * i + 2]);
    }
    out3[0] = cnt;
    out3[1] = lo;
    out3[2] = hi;
    return CAE_OK;
}

int cae_normalise_pack_rows(const float* src, int64_t n, int c_src, int64_t hw, float* dst, int c_dst, int c_off,
                            float vmin, float range, int enable, const int32_t* dst_row_dev, void* hip_stream) {
    if (!src || !dst || n < 1 || c_src < 1 || hw < 1 || c_off < 0 || c_off + c_src > c_dst)
        return fail(CAE_ERR_ARG, "cae_normalise_pack: bad argument");
    if (n > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_normalise_pack: more than 2^31 - 1 rows");
    const long long total = (long long)n * c_src * hw;
    const int blocks = (int)ceil_capped(total, 256 * 8, 8192);
    hipLaunchKernelGGL(k_normalise_pack, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, src, total, c_src,
                       (long long)hw, dst, c_dst, c_off, vmin, range, enable, (const int*)dst_row_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_normalise_pack(const float* src, int64_t n, int c_src, int64_t hw, float* dst, int c_dst, int c_off,
                       float vmin, float range, int enable, void* hip_stream) {
    return cae_normalise_pack_rows(src, n, c_src, hw, dst, c_dst, c_off, vmin, range, enable, nullptr, hip_stream);
}

int cae_invert_permutation(const int32_t* perm_dev, int64_t n, int32_t* inverse_dev, void* hip_stream) {
    if (!perm_dev || !inverse_dev || n < 1 || n > 0x7fffffffLL) return fail(CAE_ERR_ARG, "cae_invert_permutation: bad argument");
    hipLaunchKernelGGL(k_invert_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const int*)perm_dev, (long long)n, (int*)inverse_dev);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_denormalise_f64(const float* y, int64_t n, double vmin, double range, double* out, void* hip_stream) {
    if (!y || !out || n < 1) return fail(CAE_ERR_ARG, "cae_denormalise_f64: bad argument");
    const int blocks = (int)ceil_capped(n, 256 * 8, 8192);
    hipLaunchKernelGGL(k_denorm_f64, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, y, (long long)n, vmin, range, out);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_metric_sums(const float* y, const float* actual, const float* mask, int64_t n_inst, int64_t inst_elems,
                    double vmin, double range, double* sums, void* hip_stream) {
    if (!y || !actual || !sums || n_inst < 1 || inst_elems < 1 || n_inst > 65535)
        return fail(CAE_ERR_ARG, "cae_metric_sums: bad argument");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(sums, 0, (size_t)n_inst * 8 * sizeof(double), s));
    const int chunks = (int)ceil_capped(inst_elems, 256 * 16, 64);
    hipLaunchKernelGGL(k_metric_sums, dim3(chunks, (unsigned)n_inst), dim3(256), 0, s, y, actual, mask,
                       (long long)inst_elems, vmin, range, sums);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}

int cae_bswap32(void* x, int64_t n, void* hip_stream) {
    if (!x || n < 0 || ((uintptr_t)x & 15)) return fail(CAE_ERR_ARG, "cae_bswap32: bad argument (16-byte aligned device pointer)");
    if (n == 0) return CAE_OK;
    int blocks = (int)ceil_capped(n / 4, 256, 4096);
    if (blocks < 1) blocks = 1;         // fewer than four bytes: the tail alone
    hipLaunchKernelGGL(k_bswap32, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream, (unsigned*)x, (long long)n);
    HIP_TRY(hipGetLastError());
    return CAE_OK;
}
