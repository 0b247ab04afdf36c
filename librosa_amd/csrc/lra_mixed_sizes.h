// lra_mixed_sizes.h -- the frame lengths the mixed-radix kernels (lra_mixed.h) are instantiated for, and the host arithmetic on those lists.
// No HIP include: the host simulators (tests/hostsim) include it as the library does, so there is one copy of every list.
#pragma once

// frame lengths n_fft = 2 M, M = 2^a 3^b 5^c 7^d, served by one fused launch (everything else that is not a power of two keeps the rocFFT
// path): the 15 / 20 / 25 / 30 / 40 / 50 / 60 ms frames of 8, 16, 22.05 (rounded), 32 and 48 kHz front ends and their doubles; round 6: radix 7 for the
// 20 / 40 / 60 / 80 ms frames of 44.1 kHz (882 = 2 3^2 7^2, 1764, 2646, 3528 samples)
#define LRA_MIXED_SIZES(X) X(160) X(200) X(240) X(320) X(400) X(480) X(600) X(640) X(720) X(800) X(882) X(960) X(1000) X(1200) X(1280) X(1440) X(1600) X(1764) X(1920) X(2000) X(2400) X(2646) X(3200) X(3528) X(4800)

// INVERSE only: power-of-two frame lengths whose hop does not divide them the way the register-tiled inverse wants (n_fft / {2, 4, 8, 16}) --
// n_fft = 512 with hop 160 (25 ms windows padded to 512 at 16 kHz), 1024 with 441, ... -- take the fused gather kernel of lra_mixed.h instead of
// spec_pack + rocFFT + overlap-add (larger frames hold too few frames per workgroup for it: lra_api.hip's own / halo rule)
#define LRA_MIXED_INV_POW2(X) X(256) X(512) X(1024)

// FORWARD, fused mel only: powers of two whose register-tiled mel kernel is slower than lra_mixed.h's (n_fft 256: eight-thread frames leave the band combine to too
// few lanes -- 256 / 64 / 80 bands over 256 x 30 s: 2.02 ms against 1.04 for the bare transform; ctx option mixed_pow2_mel)
#define LRA_MIXED_FWD_POW2(X) X(128) X(256)

// the constant-Q octave kernel's frame lengths (filters.wavelet pads every octave's filters to a power of two)
#define LRA_CQT_SIZES(X) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)

namespace lra {
namespace mixed {
constexpr bool in_cqt_size_list(int n_fft) {
#define LRA_MIXED_CASE(N) \
    if (n_fft == N) return true;
    LRA_CQT_SIZES(LRA_MIXED_CASE)
#undef LRA_MIXED_CASE
    return false;
}
constexpr bool in_size_list(int n_fft) {
#define LRA_MIXED_CASE(N) \
    if (n_fft == N) return true;
    LRA_MIXED_SIZES(LRA_MIXED_CASE)
#undef LRA_MIXED_CASE
    return false;
}
constexpr bool in_fwd_pow2_list(int n_fft) {
#define LRA_MIXED_CASE(N) \
    if (n_fft == N) return true;
    LRA_MIXED_FWD_POW2(LRA_MIXED_CASE)
#undef LRA_MIXED_CASE
    return false;
}
constexpr bool in_inv_pow2_list(int n_fft) {
#define LRA_MIXED_CASE(N) \
    if (n_fft == N) return true;
    LRA_MIXED_INV_POW2(LRA_MIXED_CASE)
#undef LRA_MIXED_CASE
    return false;
}
// the smallest size of LRA_MIXED_SIZES that is at least `need`, or 0 where none is
constexpr int smallest_size_at_least(int need) {
    int best = 0;
#define LRA_MIXED_CASE(N) \
    if (N >= need && (best == 0 || N < best)) best = N;
    LRA_MIXED_SIZES(LRA_MIXED_CASE)
#undef LRA_MIXED_CASE
    return best;
}
}  // namespace mixed
}  // namespace lra
