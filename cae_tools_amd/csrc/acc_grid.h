// acc_grid.h — the fixed accumulation grids of every cross-workgroup fp64 sum (bitwise reproducible training steps).
//
// A header FRAGMENT without an include guard: it holds only force-inlined device templates and is included inside the
// namespace of its includer - device_common.h (namespace cae; unet_engine.hip compiles that file once more inside a
// namespace of its own) and kernels_unet.h (namespace unet, for the UNET, VAE and Linear engines).  Including it
// twice into ONE namespace is a compile error, not a silent second definition.

// ---- order-independent accumulation -----------------------------------------------------------------------------------------
// Every sum over workgroups (and the few over waves that go through LDS atomics) is a set of fp64 atomic adds whose ORDER
// differs from run to run.  fp64 addition is not associative, so such a sum is reproducible to ~1e-16 but not bitwise - and
// one last bit of an fp64 sum is, every few thousand values, one last bit of the fp32 number derived from it.  Here every
// addend is first rounded to a fixed absolute grid q (a power of two per kind of quantity).  A sum of multiples of q is EXACT
// in fp64 as long as it stays below 2^53 q, exact addition is associative, and the result therefore does not depend on the
// order the atomics arrive in: the training step is bitwise reproducible from run to run (tests/test_reproducible_gpu.py),
// for two fp64 instructions per atomic.  The grids:
//   ACC_STAT  sum y, sum y^2 of a BatchNorm layer (table slots 0, 1): q = 2^-28 (3.7e-9), exact while |sum| < 2^25 = 3.4e7
//             (N E[y^2] of a layer: 2e6 values of order 1 at the benchmark size);
//   ACC_GRAD  everything gradient-sized - sum g and sum g x_hat of BatchNorm backward (slots 2, 3), weight and bias gradients,
//             the loss: q = 2^-50 (8.9e-16), exact while |sum| < 8;
//   ACC_PLANE moments of one image plane that are read back as sums, not divided by the count first - the per-(b, c) loss
//             moments of the UNET (up to 2^16 masked pixels), the MS-SSIM / contrast sums of the VAE (2^18 pixels of a 512 x 512
//             plane), the VAE's KL sum: q = 2^-32 (2.3e-10), exact while |sum| < 2^21 = 2.1e6 (2^18 values of |v| <= 8).
//             (Used by the UNET, VAE and Linear engines only.)
// A sum that leaves its window is not wrong, it merely rounds as fp64 sums always did (reproducible to ~1e-16 again).  The
// resolution costs at most 0.5 q per addend, and an addend covers >= 16 values, so E[y^2] and the mean carry an absolute error
// of at most 1.2e-10: on the variance of a layer with outputs of order 1 that is 1e-10 relative; in the worst case (a layer
// whose variance is far below BatchNorm's eps = 1e-5) 1 / sqrt(var + eps) moves by 6e-6.  Gradient sums: 4e-16 per addend.
// Plane moments: 1.2e-10 per addend on sums of order 1e3..1e5, below 1e-13 relative.
enum AccKind : int { ACC_STAT = 0, ACC_GRAD = 1, ACC_PLANE = 2 };
template <int KIND>
__device__ __forceinline__ double acc_grid(double v) {
    constexpr double S = KIND == ACC_STAT ? 268435456.0 : KIND == ACC_GRAD ? 1125899906842624.0 : 4294967296.0;   // 2^28, 2^50, 2^32
    return __dmul_rn(rint(__dmul_rn(v, S)), 1.0 / S);
}
template <int KIND>
__device__ __forceinline__ void acc_add(double* p, double v) {
    atomicAdd(p, acc_grid<KIND>(v));
}
