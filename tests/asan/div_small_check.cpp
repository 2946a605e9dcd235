// div_small_check.cpp - the declared domain of div_small (cae_tools_amd/csrc/device_common.h), checked exhaustively on the CPU.
// Host only, no GPU and no HIP header: the expression is copied below (tests/test_hand_specs_cpu.py compares the copy and the
// two constants with the header's text before it compiles this file).  Compile with -ffp-contract=off: the device code is a
// conversion, an fp32 add and an fp32 multiply, nothing a fused multiply-add could replace.
//
// (n + 0.5f) * inv_d is monotonic in n (every fp32 operation involved is), so for a given d the quotient is right at every n
// of a run [k d, (k + 1) d - 1] if it is right at both ends: the check visits n = k d - 1 and n = k d only.
//
//     div_small_check            exit 0 and "div_small exact on ..." when no quotient on the declared domain is wrong;
//                                also prints the first wrong quotient beyond either limit
#include <cstdint>
#include <cstdio>

static inline int div_small(int n, float inv_d) { return (int)(((float)n + 0.5f) * inv_d); }   // device_common.h
constexpr int kDivSmallMaxN = 1 << 22, kDivSmallMaxD = 8000;                                     // device_common.h

// first n in [from, below) at a multiple boundary of d whose quotient is wrong, or -1; *evals counts the evaluations
static int64_t first_wrong(int d, int64_t from, int64_t below, int64_t* evals) {
    const float inv_d = 1.0f / (float)d;
    for (int64_t k = from / d; k * d - 1 < below; k++) {
        for (int64_t n = k * d - 1; n <= k * d; n++) {
            if (n < from || n < 0 || n >= below) continue;
            ++*evals;
            if (div_small((int)n, inv_d) != (int)(n / d)) return n;
        }
    }
    return -1;
}

int main() {
    int64_t evals = 0;
    int wrong = 0;
    for (int d = 1; d < kDivSmallMaxD; d++) {
        const int64_t n = first_wrong(d, 0, kDivSmallMaxN, &evals);
        if (n >= 0) {
            if (wrong++ < 10) printf("WRONG n=%lld d=%d: div_small %d, n / d %lld\n", (long long)n, d, div_small((int)n, 1.0f / (float)d), (long long)(n / d));
        }
    }
    printf("checked %lld quotients: d in [1, %d), n in [0, %d)\n", (long long)evals, kDivSmallMaxD, kDivSmallMaxN);
    // beyond the limits, so that either constant is moved knowingly: the smallest n >= kDivSmallMaxN that some d of the domain
    // gets wrong, and the smallest d >= kDivSmallMaxD that gets some n of the domain wrong
    int64_t beyond_n = -1, unused = 0;
    int beyond_n_d = 0;
    for (int d = 1; d < kDivSmallMaxD; d++) {
        const int64_t n = first_wrong(d, kDivSmallMaxN, beyond_n >= 0 ? beyond_n : 4 * (int64_t)kDivSmallMaxN, &unused);
        if (n >= 0) { beyond_n = n; beyond_n_d = d; }
    }
    if (beyond_n >= 0) printf("first wrong beyond n: n=%lld d=%d\n", (long long)beyond_n, beyond_n_d);
    else printf("first wrong beyond n: none below %lld\n", 4 * (long long)kDivSmallMaxN);
    int beyond_d = -1;
    int64_t beyond_d_n = -1;
    for (int d = kDivSmallMaxD; d < 4 * kDivSmallMaxD && beyond_d < 0; d++) {
        const int64_t n = first_wrong(d, 0, kDivSmallMaxN, &unused);
        if (n >= 0) { beyond_d = d; beyond_d_n = n; }
    }
    if (beyond_d >= 0) printf("first wrong beyond d: d=%d n=%lld\n", beyond_d, (long long)beyond_d_n);
    else printf("first wrong beyond d: none below %d\n", 4 * kDivSmallMaxD);
    if (wrong) {
        printf("div_small WRONG at %d divisors of its declared domain\n", wrong);
        return 1;
    }
    printf("div_small exact on its declared domain\n");
    return 0;
}
