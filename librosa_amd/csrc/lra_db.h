// lra_db.h -- the decibel arithmetic of power_to_db / amplitude_to_db (librosa/core/spectrum.py:1735-1883, 1946-2038), shared by the
// elementwise scaling and MFCC kernels (lra_post.h) and the onset-strength kernels (lra_onset.h), which apply it while they read a power
// spectrogram.  Self-contained so that the host simulator can include it (-DLRA_POSTSIM: the simulator defines the HIP qualifiers).
#pragma once

#ifndef LRA_POSTSIM
#include <hip/hip_runtime.h>
#endif

namespace lra {

template <class T> __device__ __forceinline__ T ten_log10(T v) { return (T)10 * log10(v); }
template <> __device__ __forceinline__ float ten_log10<float>(float v) { return 10.0f * log10f(v); }

template <class T> struct DbArgs {
    T amin;               // power domain (the host squares amplitude_to_db's amin)
    T ref_scalar;         // |ref| when ref_items == nullptr (input domain: squared here for amplitudes)
    const T* ref_items;   // per-item |reference| values (input domain), or nullptr
    const T* item_max;    // per-item max of |x| (input domain), or nullptr when top_db is None
    T top_db;
};

template <class T> __device__ __forceinline__ T db_of(T mag, T amin, T ref_db) { return ten_log10<T>(mag > amin ? mag : amin) - ref_db; }

template <class T> __device__ __forceinline__ void db_item_constants(const DbArgs<T>& d, long long item, bool amp, T& ref_db, T& floor_db) {
    T ref = d.ref_items ? d.ref_items[item] : d.ref_scalar;
    if (amp) ref = ref * ref;
    ref_db = ten_log10<T>(ref > d.amin ? ref : d.amin);
    floor_db = -INFINITY;
    if (d.item_max) {
        T mx = d.item_max[item];
        if (amp) mx = mx * mx;
        floor_db = db_of<T>(mx, d.amin, ref_db) - d.top_db;  // log10 is monotone: max of the logs = log of the max
    }
}

}  // namespace lra
