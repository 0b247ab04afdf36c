// knnsim.cpp -- runs the neighbour-graph kernel bodies of librosa_amd/csrc/lra_knn.h on host fibres (tests/hostsim/simshim.h), with the launch
// geometry of the library's own host function (knn::geometry) and its sequence of launches (lra_knn_inst.hip).
//
// The waves of knn_select walk different numbers of candidates, so they do not reach the workgroup barrier after the same number of wave
// meetings: the barrier here counts arrivals instead of taking one sweep over the fibres for one phase.
//
// TEST INFRASTRUCTURE ONLY.  Built by tests/hostsim_util.py (sim_lib) into tests/hostsim/_knnsim.so.
// Never linked into, imported by, or used as a fallback for the product library.
#define LRA_SIM_FIBRES 1
#include "simshim.h"

namespace lra {
namespace dtw {
void dtw_wave_sync() { sim::meet_wave(); }
void dtw_flag_or(int* word, int bits) { *word |= bits; }
}  // namespace dtw
namespace knn {
static unsigned g_arrived = 0;
static unsigned long long g_phase = 0;
void knn_block_sync() {
    const unsigned long long phase = g_phase;
    if (++g_arrived == blockDim.x) {
        g_arrived = 0;
        ++g_phase;
    }
    sim::meet_block();   // (at least one hand-over, as every barrier of the shim)
    while (g_phase == phase) sim::meet_block();
}
void knn_wave_sync() { sim::meet_wave(); }
unsigned long long knn_ballot(int pred) { return sim::wave_ballot(pred); }
void knn_status_or(int* word, int bits) { *word |= bits; }
void knn_status_min(int* word, int v) { if (v < *word) *word = v; }
void knn_lds_add(int* word, int v) { *word += v; }
}  // namespace knn
}  // namespace lra

#include "../../librosa_amd/csrc/lra_knn.h"

namespace lra {
namespace knn {
// the device's butterfly as one meeting of the wave: every lane folds the 64 posted pairs in lane order
void knn_wave_max(double* d, int* i, int* p) {
    struct Slot { double d; int i, p; };
    const Slot r = sim::wave_reduce(Slot{*d, *i, *p}, [](Slot a, Slot b) { return b.p >= 0 && (a.p < 0 || knn_less(a.d, a.i, b.d, b.i)) ? b : a; });
    *d = r.d;
    *i = r.i;
    *p = r.p;
}
}  // namespace knn
}  // namespace lra

using namespace lra::knn;

static unsigned blocks_of(long long count, int nt) { return (unsigned)((count + nt - 1) / nt); }

static void fill_value(Value* v, int mode, int bw_mode, double bw_scalar, int bw_on_device, const void* sigma, const void* matrix, long long m, void* work) {
    v->mode = mode;
    v->bw_mode = bw_mode;
    v->bw_scalar = bw_scalar;
    v->bw_ptr = bw_on_device ? (const double*)((const char*)work + 8) : nullptr;
    v->sigma = (const double*)sigma;
    v->matrix = (const double*)matrix;
    v->m = m;
}

extern "C" {
long long knnsim_lds_bytes(int rows, int tile, int k) { return geometry(rows, tile, k).lds; }

// out = {rows, tile, lds, workgroups}
void knnsim_geometry(int rows, int tile, int k, long long n, long long* out) {
    const Geometry g = geometry(rows, tile, k);
    out[0] = g.rows;
    out[1] = g.tile;
    out[2] = g.lds;
    out[3] = g.lds ? (n + g.rows - 1) / g.rows : 0;
}

// the arguments of lra_knn_select_exec, host pointers; -1 for a refused call
int knnsim_select(const void* Q, const void* R, int is_f64, long long d, long long n, long long m, int metric, int k, long long width, int skip_zero, int rows, int tile, int* cnt, int* idx,
                  double* dist) {
    SelectArgs a{};
    a.Q = Q;
    a.R = R;
    a.f64 = is_f64;
    a.metric = metric;
    a.d = d;
    a.n = n;
    a.m = m;
    a.k = k;
    a.width = width;
    a.skip_zero = skip_zero;
    a.cnt = cnt;
    a.idx = idx;
    a.dist = dist;
    a.g = geometry(rows, tile, k);
    if (a.g.lds == 0 || n < 1 || m < 1 || d < 1) return -1;
    std::memset(g_postsim_dyn_lds, 0xA5, sizeof(g_postsim_dyn_lds));
    const SelectKernel kern = select_kernel(metric);
    if (!kern) return -1;
    run_grid((unsigned)((n + a.g.rows - 1) / a.g.rows), kNT, [=] { kern(a); });
    const SortArgs s{n, k, cnt, idx, dist};
    std::memset(g_postsim_dyn_lds, 0xA5, sizeof(g_postsim_dyn_lds));
    run_grid((unsigned)n, kSortNT, [=] { knn_sort_rows(s); });
    return 0;
}

void knnsim_mutual(long long n, int k, const int* cnt, const int* idx, const double* dist, int sym, int drop_zero, uint8_t* keep) {
    const MutualArgs a{n, k, cnt, idx, dist, sym, drop_zero, keep};
    run_grid_serial(blocks_of(n * k, kRowNT), kRowNT, [=] { knn_mutual(a); });
}

// work: {int status, int first_empty, double bandwidth, long long total}
void knnsim_bandwidth(long long n, int k, const int* cnt, const double* dist, const uint8_t* keep, int add_self, int bandwidth_k, int median, double* dist_to_k, double* avg, void* work) {
    int* status = (int*)work;
    status[0] = 0;
    status[1] = 0x7fffffff;
    const BandwidthArgs a{n, k, cnt, dist, keep, add_self, bandwidth_k, dist_to_k, avg, status};
    std::memset(g_postsim_dyn_lds, 0xA5, sizeof(g_postsim_dyn_lds));
    run_grid((unsigned)n, kRowNT, [=] { knn_bandwidth(a); });
    if (median) {
        const MedianArgs md{dist_to_k, n, (double*)((char*)work + 8), status};
        run_grid(1, kMedNT, [=] { knn_median(md); });
    }
}

// np.nanmedian(v) into work + 8, the status word at work
void knnsim_median(const double* v, long long n, void* work) {
    int* status = (int*)work;
    status[0] = 0;
    const MedianArgs md{v, n, (double*)((char*)work + 8), status};
    run_grid(1, kMedNT, [=] { knn_median(md); });
}

int knnsim_bw_check(const double* matrix, long long count) {
    int status = 0;
    const CheckArgs a{matrix, count, &status};
    run_grid_serial(blocks_of(count, kRowNT), kRowNT, [=] { knn_bw_check(a); });
    return status;
}

// the arguments of lra_knn_emit_exec; returns the entry count of the compressed arrays
long long knnsim_emit(long long n, long long m, int k, const int* cnt, const int* idx, const double* dist, const uint8_t* keep, int self, int mode, int bw_mode, double bw_scalar,
                      int bw_on_device, const void* sigma, const void* matrix, void* work, int* counts, int* indptr, int* indices, void* data, void* dense) {
    EmitArgs a{};
    fill_value(&a.val, mode, bw_mode, bw_scalar, bw_on_device, sigma, matrix, m, work);
    a.n = n;
    a.m = m;
    a.k = k;
    a.cnt = cnt;
    a.idx = idx;
    a.dist = dist;
    a.keep = keep;
    a.self = self;
    a.counts = counts;
    a.indptr = dense ? nullptr : indptr;
    a.indices = indices;
    a.data = data;
    a.dense = dense;
    a.total = (long long*)((char*)work + 16);
    if (dense) {
        std::memset(dense, 0, (size_t)n * (size_t)m * (mode == kConnectivity ? 1 : 8));
    } else {
        run_grid_serial(blocks_of(n, kRowNT), kRowNT, [=] { knn_count(a); });
        run_grid(1, kRowNT, [=] { knn_scan(a); });
    }
    run_grid_serial(blocks_of(n, kRowNT), kRowNT, [=] { knn_emit(a); });
    return dense ? 0 : *a.total;
}

void knnsim_dense(const void* Q, const void* R, int is_f64, long long d, long long n, long long m, int metric, long long width, int self, int mode, int bw_mode, double bw_scalar,
                  int bw_on_device, const void* sigma, const void* matrix, void* work, void* out) {
    DenseArgs a{};
    fill_value(&a.val, mode, bw_mode, bw_scalar, bw_on_device, sigma, matrix, m, work);
    a.Q = Q;
    a.R = R;
    a.f64 = is_f64;
    a.metric = metric;
    a.d = d;
    a.n = n;
    a.m = m;
    a.width = width;
    a.self = self;
    a.out = out;
    run_grid((unsigned)(((n + kDenseTile - 1) / kDenseTile) * ((m + kDenseTile - 1) / kDenseTile)), kDenseNT, [=] { knn_dense(a); });
}
}
