// tools/sweep_fronts.hip -- do the eight XCDs' fronts drift apart inside one long streaming launch, and does an order that
// keeps them together (or pieces staggered over two queues) beat launching in pieces?  Stand-alone: seeded data, HIP-event
// timing, every candidate checked against the natural order's result before it is timed.
//   hipcc -O3 --offload-arch=gfx950 tools/sweep_fronts.hip -o tools/bin/sweep_fronts
//   tools/bin/sweep_fronts <drift table> <sweep table>      (profiles/front_drift.txt, profiles/sweep_fronts.txt)
// The 2R+1W f32 add (nt loads and stores, workgroups of 1024 = one 16 KiB tile of each stream) at 2^26, 2^28, 2^30 elements:
//   A     one launch, natural order
//   B     the library's rule (internal.h: piece_for): halves at 2^28, pieces of 2^24 vectors above
//   aC    one launch, tile = remap(blockIdx.x): class b % 8 takes C consecutive tiles out of every group of 8 C (C = 2 .. 256;
//         C = 1 is A, C = nb / 8 is sweep_perm's xcd-chunked); identity on the ragged end
//   aC+B  the same order inside B's pieces
//   pieces of 2^23 / 2^24 / 2^25 in natural order and with C = 8, 32, 64 inside: the piece_for table again
//   bP    pieces of P = 2^23, 2^24, 2^25 vectors, even ones on one stream and odd ones on a second, the first one half-size;
//         no edges between pieces, one fork edge before and one join edge after
// and, head to head, ten alternating rounds of B against the best candidate, judged by the rule a gain has to pass;
// then the same candidates for the 1R+1W a*s stream (workgroups of 256, as the library launches it; C counts 16 KiB all the
// same) and for the fused add+sum's mix, modelled as the add plus one 4-byte store per workgroup.
// Stamp mode: lane 0 of every workgroup stores wall_clock64() at entry into ts[blockIdx.x] (a buffer of its own).  Blocks b and
// b + 8 share an XCD; for 64 instants across the launch the table gives the tile each class b % 8 has reached and the spread
// between the slowest and the fastest class in MiB of each stream.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// class b % 8 takes C = 2^lc consecutive tiles out of every group of 8 C; blocks from `whole` (the last whole group's end) on keep their place
__host__ __device__ inline unsigned remap(unsigned b, unsigned lc, unsigned whole) {
    if (lc == 0 || b >= whole) return b;
    const unsigned r = b & ((8u << lc) - 1);
    return (b - r) + ((r & 7u) << lc) + (r >> 3);
}

// KIND 0: c = a + b;  1: c = a * s;  2: c = a + b and one 4-byte store per workgroup (the fused op+sum's partial)
template <int KIND, int BLOCK, bool STAMP>
__global__ __launch_bounds__(BLOCK) void stream_k(const f4* __restrict__ a, const f4* __restrict__ b, f4* __restrict__ c, float s, float* __restrict__ partial,
                                                  unsigned lc, unsigned whole, u64* __restrict__ ts) {
    if (STAMP && threadIdx.x == 0) ts[blockIdx.x] = wall_clock64();
    const unsigned t = remap(blockIdx.x, lc, whole);
    const size_t i = (size_t)t * BLOCK + threadIdx.x;
    f4 v = __builtin_nontemporal_load(a + i);
    if (KIND == 1) v = v * s; else v = v + __builtin_nontemporal_load(b + i);
    __builtin_nontemporal_store(v, c + i);
    if (KIND == 2 && threadIdx.x == 0) partial[t] = v.x;
}
__global__ void init_k(float* p, size_t n, unsigned seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u ^ (unsigned)(i >> 32) ^ seed; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        p[i] = (float)(h >> 8) * (1.0f / 16777216.0f) - 0.5f;
    }
}
__global__ void diff_k(const unsigned* x, const unsigned* y, size_t n, unsigned* bad) {
    unsigned mine = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) mine += x[i] != y[i];
    if (mine) atomicAdd(bad, mine);
}

struct Variant { std::string name; int type; unsigned lc; size_t piece; std::vector<double> pct; };  // type 0: in order on one stream (piece 0: one launch); 1: two streams
struct Launch { size_t v0, nv; int q; };
struct Ctx { float *a, *b, *c, *ref, *partial; u64* ts; unsigned* bad; hipStream_t q[2]; hipEvent_t fork, join; };

size_t rule_b(size_t n_vec, int kind) {  // internal.h: piece_for
    if (kind == 1) return n_vec > ((size_t)1 << 27) ? (size_t)1 << 25 : 0;
    return n_vec > ((size_t)1 << 26) ? (size_t)1 << 24 : n_vec > ((size_t)1 << 25) ? (size_t)1 << 25 : 0;
}
std::vector<Launch> plan(const Variant& v, size_t n_vec) {
    std::vector<Launch> ls;
    if (v.piece == 0 || v.piece >= n_vec) { ls.push_back({0, n_vec, 0}); return ls; }
    size_t v0 = 0; int k = 0;
    while (v0 < n_vec) {
        size_t nv = std::min(n_vec - v0, (v.type == 1 && k == 0) ? v.piece / 2 : v.piece);
        ls.push_back({v0, nv, v.type == 1 ? (k & 1) : 0}); v0 += nv; ++k;
    }
    return ls;
}
template <int KIND, int BLOCK, bool STAMP>
void issue_t(const Ctx& x, const Variant& v, const std::vector<Launch>& ls) {
    const unsigned lc = v.lc ? v.lc + (BLOCK == 256 ? 2 : 0) : 0;  // C counts 16 KiB of each stream
    bool two = false; for (auto& l : ls) two |= l.q == 1;
    if (two) { CK(hipEventRecord(x.fork, x.q[0])); CK(hipStreamWaitEvent(x.q[1], x.fork, 0)); }
    for (auto& l : ls) {
        const unsigned nb = (unsigned)(l.nv / BLOCK), whole = lc ? nb & ~((8u << lc) - 1) : 0;
        stream_k<KIND, BLOCK, STAMP><<<nb, BLOCK, 0, x.q[l.q]>>>((const f4*)x.a + l.v0, (const f4*)x.b + l.v0, (f4*)x.c + l.v0, 1.25f, x.partial + l.v0 / BLOCK, lc, whole,
                                                                 x.ts + l.v0 / BLOCK);
    }
    if (two) { CK(hipEventRecord(x.join, x.q[1])); CK(hipStreamWaitEvent(x.q[0], x.join, 0)); }
}
void issue(const Ctx& x, const Variant& v, const std::vector<Launch>& ls, int kind, bool stamp) {
    if (kind == 0) { if (stamp) issue_t<0, 1024, true>(x, v, ls); else issue_t<0, 1024, false>(x, v, ls); }
    else if (kind == 1) { if (stamp) issue_t<1, 256, true>(x, v, ls); else issue_t<1, 256, false>(x, v, ls); }
    else { if (stamp) issue_t<2, 1024, true>(x, v, ls); else issue_t<2, 1024, false>(x, v, ls); }
}
double time_ms(const Ctx& x, const Variant& v, const std::vector<Launch>& ls, int kind, bool stamp, int reps) {
    static hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!e0) { CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); }
    issue(x, v, ls, kind, stamp);
    CK(hipEventRecord(e0, x.q[0])); for (int i = 0; i < reps; ++i) issue(x, v, ls, kind, stamp); CK(hipEventRecord(e1, x.q[0])); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    return ms / reps;
}

// the fronts of one stamped run: for 64 instants, how far each class b % 8 of each launch has come
void drift_table(FILE* f, const Ctx& x, const Variant& v, const std::vector<Launch>& ls, int block, double clock_khz, const char* what) {
    size_t nblk = 0; for (auto& l : ls) nblk = std::max(nblk, (l.v0 + l.nv) / block);
    std::vector<u64> ts(nblk);
    CK(hipMemcpy(ts.data(), x.ts, nblk * sizeof(u64), hipMemcpyDeviceToHost));
    const u64 t0 = *std::min_element(ts.begin(), ts.end()), t1 = *std::max_element(ts.begin(), ts.end());
    const double tile_mib = block * 16.0 / (1 << 20);
    std::vector<std::vector<std::vector<u64>>> cls(ls.size(), std::vector<std::vector<u64>>(8));  // [launch][class] -> sorted entry times
    for (size_t k = 0; k < ls.size(); ++k) {
        const size_t b0 = ls[k].v0 / block, nb = ls[k].nv / block;
        for (size_t b = 0; b < nb; ++b) cls[k][b & 7].push_back(ts[b0 + b]);
        for (auto& c : cls[k]) std::sort(c.begin(), c.end());
    }
    fprintf(f, "# %s: %s, %zu launch(es), first to last workgroup entry %.1f us\n", what, v.name.c_str(), ls.size(), (double)(t1 - t0) / clock_khz * 1e3);
    fprintf(f, "#   t_us  started   in-flight launch: tiles started by class 0..7 (of its share)                          spread_tiles  spread_MiB  | worst launch MiB\n");
    double worst_all = 0, at_worst = 0;
    for (int s = 0; s < 64; ++s) {
        const u64 t = t0 + (u64)((s + 0.5) / 64 * (double)(t1 - t0));
        size_t started = 0; double worst = 0; int shown = -1; size_t p[8] = {0}; size_t sp_shown = 0;
        for (size_t k = 0; k < ls.size(); ++k) {
            size_t q[8], lo = ~(size_t)0, hi = 0, sum = 0, full = 0;
            for (int c = 0; c < 8; ++c) { q[c] = std::upper_bound(cls[k][c].begin(), cls[k][c].end(), t) - cls[k][c].begin(); lo = std::min(lo, q[c]); hi = std::max(hi, q[c]); sum += q[c]; full += cls[k][c].size(); }
            started += sum;
            if (sum == 0 || sum == full) continue;  // not begun, or all in
            const double mib = (double)(hi - lo) * 8 * tile_mib;
            worst = std::max(worst, mib);
            if (shown < 0) { shown = (int)k; memcpy(p, q, sizeof p); sp_shown = hi - lo; }
        }
        if (worst > worst_all) { worst_all = worst; at_worst = (double)(t - t0) / clock_khz * 1e3; }
        fprintf(f, "%8.1f %8zu   #%-3d", (double)(t - t0) / clock_khz * 1e3, started, shown);
        for (int c = 0; c < 8; ++c) fprintf(f, " %7zu", p[c]);
        fprintf(f, "   %8zu  %9.2f  | %9.2f\n", sp_shown * 8, (double)sp_shown * 8 * tile_mib, worst);
    }
    fprintf(f, "# %s: %s: largest spread %.2f MiB of each stream, at %.1f us\n\n", what, v.name.c_str(), worst_all, at_worst);
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <drift table> <sweep table>\n", argv[0]); return 2; }
    FILE* fd = fopen(argv[1], "w"); FILE* fs = fopen(argv[2], "w");
    if (!fd || !fs) { perror("open"); return 2; }
    const size_t nmax = (size_t)1 << 30;
    int khz = 0; CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
    const double clock_khz = khz > 0 ? khz : 100000.0;
    Ctx x;
    CK(hipMalloc(&x.a, nmax * 4)); CK(hipMalloc(&x.b, nmax * 4)); CK(hipMalloc(&x.c, nmax * 4)); CK(hipMalloc(&x.ref, nmax * 4));
    CK(hipMalloc(&x.partial, (nmax / 4 / 256) * 4)); CK(hipMalloc(&x.ts, (nmax / 4 / 256) * sizeof(u64))); CK(hipMalloc(&x.bad, 4));
    CK(hipStreamCreateWithFlags(&x.q[0], hipStreamNonBlocking)); CK(hipStreamCreateWithFlags(&x.q[1], hipStreamNonBlocking));
    CK(hipEventCreateWithFlags(&x.fork, hipEventDisableTiming)); CK(hipEventCreateWithFlags(&x.join, hipEventDisableTiming));
    init_k<<<8192, 256>>>(x.a, nmax, 0x9e3779b9u); init_k<<<8192, 256>>>(x.b, nmax, 0x85ebca6bu); CK(hipDeviceSynchronize());
    fprintf(fs, "# tools/sweep_fronts.hip: %% of 8 TB/s over 5 alternating rounds of 10 back-to-back operators each (mean, min, max), HIP events; wall clock %.0f kHz\n", clock_khz);
    fprintf(fd, "# tools/sweep_fronts.hip, stamp mode: lane 0 of each workgroup stores wall_clock64() at entry; class = blockIdx.x %% 8 (one XCD each)\n\n");

    const char* kind_name[3] = {"2R+1W f32 add, workgroups of 1024", "1R+1W a*s, workgroups of 256", "2R+1W add + one partial per workgroup (fused add+sum's mix), workgroups of 1024"};
    for (int kind = 0; kind < 3; ++kind) for (int lg : {26, 28, 30}) {
        const size_t n = (size_t)1 << lg, n_vec = n / 4;
        const int block = kind == 1 ? 256 : 1024;
        const double bytes = (kind == 1 ? 8.0 : 12.0) * n;
        std::vector<Variant> vs;
        vs.push_back({"A one launch", 0, 0, 0, {}});
        const size_t pb = rule_b(n_vec, kind);
        vs.push_back({pb ? "B pieces of 2^" + std::to_string(__builtin_ctzll(pb)) : "B (= A here)", 0, 0, pb, {}});
        for (unsigned lc = 1; lc <= 8; ++lc) vs.push_back({"a C=" + std::to_string(1u << lc), 0, lc, 0, {}});
        if (pb) for (unsigned lc = 1; lc <= 8; ++lc) vs.push_back({"a C=" + std::to_string(1u << lc) + " in B's pieces", 0, lc, pb, {}});
        for (int lp : {23, 24, 25}) if (((size_t)1 << lp) < n_vec && ((size_t)1 << lp) != pb) {  // the piece_for table again, with and without the new order
            vs.push_back({"pieces of 2^" + std::to_string(lp), 0, 0, (size_t)1 << lp, {}});
            for (unsigned lc : {3u, 5u, 6u}) vs.push_back({"a C=" + std::to_string(1u << lc) + " in pieces of 2^" + std::to_string(lp), 0, lc, (size_t)1 << lp, {}});
        }
        for (int lp : {23, 24, 25}) if (((size_t)1 << lp) < n_vec) vs.push_back({"b two queues, pieces of 2^" + std::to_string(lp), 1, 0, (size_t)1 << lp, {}});
        // every candidate computes what A computes
        Variant& A = vs[0];
        CK(hipMemsetAsync(x.c, 0, n * 4, x.q[0])); issue(x, A, plan(A, n_vec), kind, false); CK(hipStreamSynchronize(x.q[0]));
        CK(hipMemcpyAsync(x.ref, x.c, n * 4, hipMemcpyDeviceToDevice, x.q[0]));
        for (auto& v : vs) {
            CK(hipMemsetAsync(x.c, 0, n * 4, x.q[0])); CK(hipMemsetAsync(x.bad, 0, 4, x.q[0]));
            issue(x, v, plan(v, n_vec), kind, false);
            diff_k<<<4096, 256, 0, x.q[0]>>>((const unsigned*)x.c, (const unsigned*)x.ref, n, x.bad); CK(hipStreamSynchronize(x.q[0]));
            unsigned bad; CK(hipMemcpy(&bad, x.bad, 4, hipMemcpyDeviceToHost));
            if (bad) { fprintf(stderr, "%s at 2^%d: %u words differ from the natural order's result\n", v.name.c_str(), lg, bad); return 1; }
        }
        for (int round = 0; round < 5; ++round) for (auto& v : vs) v.pct.push_back(bytes / (time_ms(x, v, plan(v, n_vec), kind, false, 10) * 1e-3) / 8e12 * 100);
        fprintf(fs, "\n## %s, N = 2^%d (%zu MiB per stream)\n", kind_name[kind], lg, n * 4 >> 20);
        int best_a = -1, best_b = -1; double ma = 0, mb = 0, mB = 0;
        for (size_t i = 0; i < vs.size(); ++i) {
            auto& p = vs[i].pct; double sum = 0; for (double q : p) sum += q;
            const double mean = sum / p.size();
            fprintf(fs, "%-40s %6.2f  (%6.2f .. %6.2f)   %8.1f us\n", vs[i].name.c_str(), mean, *std::min_element(p.begin(), p.end()), *std::max_element(p.begin(), p.end()), bytes / (mean / 100 * 8e12) * 1e6);
            if (i == 1) mB = mean;
            if (vs[i].name[0] == 'a' && mean > ma) { ma = mean; best_a = (int)i; }
            if (vs[i].name[0] == 'b' && mean > mb) { mb = mean; best_b = (int)i; }
        }
        const int best = mb > ma ? best_b : best_a;
        fprintf(fs, "best of (a): %s %+.2f %% of B;  best of (b): %s %+.2f %% of B\n", vs[best_a].name.c_str(), (ma / mB - 1) * 100, best_b >= 0 ? vs[best_b].name.c_str() : "-", best_b >= 0 ? (mb / mB - 1) * 100 : 0.0);
        {   // head to head, by the rule a gain has to pass: every round of the candidate above every round of B, mean gain >= 3 x B's own spread
            double b_lo = 1e9, b_hi = 0, c_lo = 1e9, b_sum = 0, c_sum = 0;
            fprintf(fs, "head to head, 10 alternating rounds of 20 operators, B / %s:", vs[best].name.c_str());
            for (int round = 0; round < 10; ++round) {
                const double pb_ = bytes / (time_ms(x, vs[1], plan(vs[1], n_vec), kind, false, 20) * 1e-3) / 8e12 * 100;
                const double pc_ = bytes / (time_ms(x, vs[best], plan(vs[best], n_vec), kind, false, 20) * 1e-3) / 8e12 * 100;
                fprintf(fs, "  %.2f/%.2f", pb_, pc_);
                b_lo = std::min(b_lo, pb_); b_hi = std::max(b_hi, pb_); c_lo = std::min(c_lo, pc_); b_sum += pb_; c_sum += pc_;
            }
            fprintf(fs, "\n  B %.2f (spread %.2f), candidate %.2f: gain %+.2f points = %.1f x B's spread; every round above every round of B: %s\n", b_sum / 10, b_hi - b_lo, c_sum / 10,
                    (c_sum - b_sum) / 10, (c_sum - b_sum) / 10 / (b_hi - b_lo), c_lo > b_hi ? "yes" : "no");
        }
        fflush(fs);
        printf("kind %d 2^%d: B %.2f %%, best a %s %.2f %%, best b %s %.2f %%\n", kind, lg, mB, vs[best_a].name.c_str(), ma, best_b >= 0 ? vs[best_b].name.c_str() : "-", mb); fflush(stdout);
        if (kind != 0) continue;
        // the fronts: A, B where it differs, and the best candidate; and what the stamp itself costs
        fprintf(fd, "## %s, N = 2^%d (%zu MiB per stream, %zu workgroups)\n", kind_name[kind], lg, n * 4 >> 20, n_vec / block);
        std::vector<int> who = {0}; if (pb) who.push_back(1); who.push_back(best);
        for (int i : who) {
            const auto ls = plan(vs[i], n_vec);
            const double plain = time_ms(x, vs[i], ls, kind, false, 10), stamped = time_ms(x, vs[i], ls, kind, true, 10);
            fprintf(fd, "# %s: %.1f us without the stamp, %.1f us with it (%+.2f %%)\n", vs[i].name.c_str(), plain * 1e3, stamped * 1e3, (stamped / plain - 1) * 100);
            CK(hipMemsetAsync(x.ts, 0, (n_vec / block) * sizeof(u64), x.q[0])); issue(x, vs[i], ls, kind, true); CK(hipStreamSynchronize(x.q[0])); CK(hipStreamSynchronize(x.q[1]));
            drift_table(fd, x, vs[i], ls, block, clock_khz, i == 0 ? "control A" : i == 1 ? "control B" : "best candidate");
        }
        fflush(fd);
    }
    fclose(fd); fclose(fs);
    return 0;
}
