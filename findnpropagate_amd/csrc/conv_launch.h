// Host side of the sparse-convolution forward, shared by spconv*.hip: the argument record every launcher takes, the refusals every
// entry point makes, and the small dispatch idioms (16-bit type code, channel pair, LDS limit).  Library-internal, host code only.
#pragma once
#include "common.h"

// What every forward launch is given.  An entry point fills it from its C arguments; a launcher takes it plus only its own extras.
struct ConvArgs {
    const void *x;         // input features and their size in bytes (32-bit buffer offsets: see fnp_fits32)
    long long x_bytes;
    const void *w;
    const int *nbr;        // (K, nbr_stride) table; null for the forms that carry their own rulebook
    int nbr_stride, K;
    const int *n_out;
    int cap;
    void *y;
    const float *scale, *shift;
    const void *residual;
    int relu, hints;
    hipStream_t stream;
};

namespace {

// The refusals the forward entry points share.  `table`: the entry reads a neighbour table (its pointer is required);
// `need_y`: feat_out is required (the split forms may write only their split).
inline bool fnp_conv_args_ok(const ConvArgs &a, long long n_in_rows, bool table = true, bool need_y = true) {
    return a.x && a.w && (a.nbr || !table) && a.n_out && (a.y || !need_y) && a.cap > 0 && a.nbr_stride >= a.cap && n_in_rows > 0 &&
           (a.scale == nullptr) == (a.shift == nullptr);
}
// a byte count the kernels' 32-bit buffer offsets reach
inline bool fnp_fits32(long long bytes) { return bytes > 0 && bytes < 0x7fffffffll; }
// no bit of `mask` set in any of the addresses (null passes)
template <typename... P> inline bool fnp_aligned(uintptr_t mask, const P *...p) { return (((uintptr_t)p | ... | (uintptr_t)0) & mask) == 0; }

// Raise a kernel's dynamic-LDS limit before its first launch.  `raised` is the caller's flag, one per kernel instantiation
// (idempotent; a race only repeats the call).
inline int fnp_raise_lds(const void *kern, int bytes, bool &raised) {
    if (raised) return FNP_OK;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return FNP_ERR_HIP;
    raised = true;
    return FNP_OK;
}

// f(TypeTag<T>{}) with T = __bf16 / _Float16 for the 16-bit type codes; FNP_ERR_ARG for any other code
template <typename T> struct TypeTag { using type = T; };
template <typename F> int fnp_dispatch16(int dtype, F &&f) {
    if (dtype == FNP_BF16) return f(TypeTag<__bf16>{});
    if (dtype == FNP_F16) return f(TypeTag<_Float16>{});
    return FNP_ERR_ARG;
}

// rc = f(ChPair<CI, CO>{}) for the listed pair that equals (Cin, Cout); false (f not called) when none does
template <int CI, int CO> struct ChPair { static constexpr int ci = CI, co = CO; };
template <typename... P> struct PairList {};
template <typename F, typename... P> bool fnp_for_pair(int Cin, int Cout, int &rc, PairList<P...>, F &&f) {
    return ((Cin == P::ci && Cout == P::co ? (rc = f(P{}), true) : false) || ...);
}
// the channel pairs of the matrix kernels, 16-bit and f32
using ConvPairs = PairList<ChPair<16, 16>, ChPair<16, 32>, ChPair<32, 32>, ChPair<32, 64>, ChPair<64, 64>, ChPair<64, 128>, ChPair<128, 128>,
                           // transposed channel pairs: the data gradients of the three channel-doubling convolutions
                           ChPair<32, 16>, ChPair<64, 32>, ChPair<128, 64>>;

}  // namespace
