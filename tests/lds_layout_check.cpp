// lds_layout_check.cpp -- stand-alone CPU check of the LDS layouts of the FFT exchanges (librosa_amd/csrc/lra_fft.h, "exchange addresses").
//
// TEST INFRASTRUCTURE ONLY.  Built and run by tests/test_lds_layout.py (g++, no GPU).  It evaluates the SAME address functions the kernels
// call -- xw_base / xw_off / xr_base / xr_off, and v2_mirror_bfly for the mirrored last pass -- for all 64 lanes and every compile-time index
// of the one-wave n_fft = 2048 float32 cores (radices 16-8-8 and 16-16-4), and counts LDS-array cycles per wave instruction by the lane groups
// and bank rules of gfx950 (scripts/lds_model.py, GROUPS): ds_read_b64 is served in two groups of 32 lanes over 64 four-byte banks,
// ds_write_b64 in four groups of 16 lanes over 32 banks; lanes of a group that want different dwords of one bank take one more cycle each.
// Output: one line per exchange, `key=value` pairs, parsed by the test.
#define LRA_HOSTSIM 1
#include "../librosa_amd/csrc/lra_dispatch.h"

#include <cstdio>
#include <map>
#include <set>
#include <vector>

using namespace lra;

struct Count {
    int insts = 0, cycles = 0, conflicts = 0;
    std::set<int> units;
    int top = 0;  // one past the last byte touched
};

// one wave instruction of 8-byte accesses: addr[lane] in bytes
static void count_b64(bool write, const int (&addr)[64], Count& c) {
    const int group = write ? 16 : 32, banks = write ? 32 : 64;
    int cyc = 0, conf = 0;
    for (int g = 0; g < 64 / group; ++g) {
        std::map<int, std::set<int>> per_bank;
        for (int l = g * group; l < (g + 1) * group; ++l)
            for (int d = 0; d < 2; ++d) per_bank[(addr[l] / 4 + d) % banks].insert(addr[l] / 4 + d);
        size_t worst = 1;
        for (auto& kv : per_bank) worst = kv.second.size() > worst ? kv.second.size() : worst;
        cyc += (int)worst;
        conf += (int)worst - 1;
    }
    c.insts += 1;
    c.cycles += cyc;
    c.conflicts += conf;
    for (int l = 0; l < 64; ++l) {
        if (addr[l] % 8 != 0 || addr[l] < 0) { std::printf("error=misaligned_or_negative_address\n"); std::exit(2); }
        c.units.insert(addr[l] / 8);
        c.top = addr[l] + 8 > c.top ? addr[l] + 8 : c.top;
    }
}

template <class Cfg, int p> static void pass_write_site(Count& c) {
    static_assert(xw_affine<Cfg, p>(), "one base per lane + immediates");
    constexpr int r = 1 << Cfg::logr(p), nb = Cfg::R >> Cfg::logr(p), SZ = (int)sizeof(typename Cfg::cplx);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < r; ++j) {
            int addr[64];
            for (int l = 0; l < 64; ++l) addr[l] = (xw_base<Cfg, p>(l) + xw_off<Cfg, p>(i, j)) * SZ;
            count_b64(true, addr, c);
        }
}
template <class Cfg, int p> static void pass_read_site(Count& c) {
    static_assert(xr_affine<Cfg, p>(), "one base per lane + immediates");
    constexpr int r = 1 << Cfg::logr(p), nb = Cfg::R >> Cfg::logr(p), SZ = (int)sizeof(typename Cfg::cplx);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < r; ++j) {
            int addr[64];
            for (int l = 0; l < 64; ++l) addr[l] = (xr_base<Cfg, p>(l) + xr_off<Cfg, p>(i, j)) * SZ;
            count_b64(false, addr, c);
        }
}
// v2_last_read: butterfly tf, then its mirror
template <class Cfg> static void mirrored_last_read_site(Count& c) {
    constexpr int p = Cfg::P - 1, r = 1 << Cfg::logr(p), SZ = (int)sizeof(typename Cfg::cplx);
    static_assert(xr_affine<Cfg, p>() && (Cfg::R >> Cfg::logr(p)) == 2, "two butterflies per lane: tf and its mirror");
    for (int j = 0; j < r; ++j)
        for (int fam = 0; fam < 2; ++fam) {
            int addr[64];
            for (int l = 0; l < 64; ++l) addr[l] = (xr_base<Cfg, p>(fam ? v2_mirror_bfly<Cfg>(l) : l) + xr_off<Cfg, p>(0, j)) * SZ;
            count_b64(false, addr, c);
        }
}

static void report(const char* plan, int exchange, int layout, int frame_bytes, const Count& w, const Count& r) {
    std::printf("plan=%s exchange=%d layout=%d write_insts=%d write_cycles=%d write_conflicts=%d read_insts=%d read_cycles=%d read_conflicts=%d units_written=%d units_read=%d sets_equal=%d "
                "footprint_bytes=%d frame_bytes=%d\n",
                plan, exchange, layout, w.insts, w.cycles, w.conflicts, r.insts, r.cycles, r.conflicts, (int)w.units.size(), (int)r.units.size(), (int)(w.units == r.units),
                w.top > r.top ? w.top : r.top, frame_bytes);
}

template <class Cfg> static void check(const char* plan) {
    static_assert(Cfg::TF == 64 && Cfg::R == 16 && Cfg::M == 1024 && Cfg::P == 3, "one wave per frame, n_fft = 2048");
    {
        Count w, r;
        pass_write_site<Cfg, 0>(w);
        pass_read_site<Cfg, 1>(r);
        report(plan, 1, xw_layout<Cfg, 0>(), Cfg::FRAME_BYTES, w, r);
        if (xw_layout<Cfg, 0>() != xr_layout<Cfg, 1>()) { std::printf("error=exchange_1_layouts_differ\n"); std::exit(2); }
    }
    if constexpr (Cfg::PLAN == 0) {  // (16-16-4: the middle -> last hand-over has a form of its own, v3_mid_write / v3_last_read)
        Count w, r;
        pass_write_site<Cfg, 1>(w);
        mirrored_last_read_site<Cfg>(r);
        report(plan, 2, xw_layout<Cfg, 1>(), Cfg::FRAME_BYTES, w, r);
        if (xw_layout<Cfg, 1>() != xr_layout<Cfg, 2>()) { std::printf("error=exchange_2_layouts_differ\n"); std::exit(2); }
        // the first-generation body reads the same exchange butterfly by butterfly (pass_read): same units
        Count r1;
        pass_read_site<Cfg, 2>(r1);
        if (r1.units != w.units) { std::printf("error=pass_read_last_reads_other_units\n"); std::exit(2); }
    }
}

int main() {
    check<CfgSel<float, 10, 0>::type>("16-8-8");
    check<CfgSel<float, 10, 6>::type>("16-16-4");
    check<MelCfgOf<CfgSel<float, 10, 0>::type>::type>("16-8-8/mel");  // (the one-wave mel kernel's workgroup shape: same frame, same layouts)
    return 0;
}
