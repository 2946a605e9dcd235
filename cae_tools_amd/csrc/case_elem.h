// case_elem.h - the element loads of the case kernels: an operand is channel 0 of the cases in one of the element kinds of
// include/cae_hip.h, and the denormalisation of a score that those kernels share (cm_denorm).  Included by
// kernels_stateless.h where they have always stood, and by the kernel headers that use them.
#pragma once
#include "device_common.h"

namespace cae {

// Element kinds (CAE_ELEM_*): 0 fp32, 1 fp32 big-endian, 2 fp64, 3 fp64 big-endian.  A big-endian
// slab is the NetCDF-3 file's bytes copied to HBM as they are; the swap happens in registers.
template <int K> struct CmElem;
template <> struct CmElem<0> { static constexpr int bytes = 4; };
template <> struct CmElem<1> { static constexpr int bytes = 4; };
template <> struct CmElem<2> { static constexpr int bytes = 8; };
template <> struct CmElem<3> { static constexpr int bytes = 8; };

template <int K>
__device__ __forceinline__ double cm_word(unsigned long long w) {
    if constexpr (K == 0) return (double)__uint_as_float((unsigned)w);
    else if constexpr (K == 1) return (double)__uint_as_float(__builtin_bswap32((unsigned)w));
    else if constexpr (K == 2) return __longlong_as_double((long long)w);
    else return __longlong_as_double((long long)__builtin_bswap64(w));
}

// element e of a case (element-aligned pointer)
template <int K>
__device__ __forceinline__ double cm_load1(const unsigned char* c, long long e) {
    if constexpr (CmElem<K>::bytes == 4) return cm_word<K>(reinterpret_cast<const unsigned*>(c)[e]);
    else return cm_word<K>(reinterpret_cast<const unsigned long long*>(c)[e]);
}

// elements e .. e+3: 16-byte loads when `vec` (the caller checked the alignment), else four scalar loads
template <int K>
__device__ __forceinline__ void cm_load4(const unsigned char* c, long long e, bool vec, double v[4]) {
    if (vec) {
        if constexpr (CmElem<K>::bytes == 4) {
            const uint4 w = *reinterpret_cast<const uint4*>(c + e * 4);
            v[0] = cm_word<K>(w.x);
            v[1] = cm_word<K>(w.y);
            v[2] = cm_word<K>(w.z);
            v[3] = cm_word<K>(w.w);
        } else {
            const ulonglong2 w0 = *reinterpret_cast<const ulonglong2*>(c + e * 8);
            const ulonglong2 w1 = *reinterpret_cast<const ulonglong2*>(c + e * 8 + 16);
            v[0] = cm_word<K>(w0.x);
            v[1] = cm_word<K>(w0.y);
            v[2] = cm_word<K>(w1.x);
            v[3] = cm_word<K>(w1.y);
        }
    } else {
        for (int j = 0; j < 4; j++) v[j] = cm_load1<K>(c, e + j);
    }
}

// The denormalised score of ds_dataset.py:131-135, vmin + (y * range) in two rounded fp64 operations as numpy forms it.
// Plain operators under the pragma: the bodies of __dadd_rn and __dmul_rn are a plain + and * that the compiler contracts
// into one v_fma_f64 wherever they are inlined, which changes the last bit unless y * range happens to be exact.
__device__ __forceinline__ double cm_denorm(double vmin, double y, double range) {
#pragma clang fp contract(off)
    const double prod = y * range;
    return vmin + prod;
}

}  // namespace cae
