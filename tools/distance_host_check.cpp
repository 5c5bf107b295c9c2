// The distance-map verification of dl4ds_amd/csrc/distance.hip, run on the CPU: the same three steps (column pass, row pass with the
// segment walk, final reduction) lane by lane and cell by cell through the functions of distance_core.h, in the kernels' own
// order (a lane's cells in ascending j, the shuffle tree over 64 lanes, the rows t, t + 256, ... per thread and the tree over 256
// threads), with every array access checked.  A stray index prints the array and the index and ends the program with status 2.
//
//   c++ -std=c++17 -O1 -ffp-contract=off -o distance_host_check tools/distance_host_check.cpp
//                                                                   (sanitizers: add -fsanitize=address,undefined -fno-sanitize-recover=all)
//   distance_host_check case.bin out.bin
//
// case.bin: int32 N, H, W, C, T, seg (columns of a row segment, 1 ... 1024), fp64 cutoff, alpha, float32 thr[T], then float32
//           y[N][H][W][C] and p[N][H][W][C].
// out.bin:  counts int64 [F][T][8], sums fp64 [F][T][7], d2_obs int32 [F][T][H][W], d2_pred int32 [F][T][H][W].
// tests/test_distance_api.py compares that with tests/distance_ref.py on every case of tests/distance_cases.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

static const int* g_lo = nullptr;
static const int* g_hi = nullptr;
static void check_access(const int* p) {
    if (p < g_lo || p >= g_hi) {
        std::fprintf(stderr, "distance_host_check: segment[%lld] is outside [0, %lld)\n", (long long)(p - g_lo), (long long)(g_hi - g_lo));
        std::exit(2);
    }
}
#define DC_CHECK_ACCESS(p) check_access(p)
#include "../dl4ds_amd/csrc/distance_core.h"

template <typename T>
struct Arr {
    std::vector<T> v;
    const char* name;
    Arr(const char* n, size_t size, T fill = T()) : v(size, fill), name(n) {}
    T& at(size_t k) {
        if (k >= v.size()) {
            std::fprintf(stderr, "distance_host_check: %s[%zu] is outside [0, %zu)\n", name, k, v.size());
            std::exit(2);
        }
        return v[k];
    }
    void write(std::FILE* f) { if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3); }
};
static void fail(const char* what) { std::fprintf(stderr, "distance_host_check: %s\n", what); std::exit(1); }

constexpr int LANES = 64, FINAL_THREADS = 256;

// lane 0 of the kernel's shuffle tree: at offset o lane l joins what lane l + o held before the step (its own beyond the wave)
static DcTerms tree64(std::vector<DcTerms> acc) {
    for (int o = LANES / 2; o > 0; o >>= 1) {
        std::vector<DcTerms> before(acc);
        for (int l = 0; l < LANES; ++l) dc_join(&acc[l], &before[l + o < LANES ? l + o : l]);
    }
    return acc[0];
}

int main(int argc, char** argv) {
    if (argc != 3) fail("usage: distance_host_check case.bin out.bin");
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) fail("cannot open the case file");
    int head[6];
    double par[2];
    if (std::fread(head, sizeof(int), 6, in) != 6 || std::fread(par, sizeof(double), 2, in) != 2) fail("short header");
    const int N = head[0], H = head[1], W = head[2], C = head[3], T = head[4], seg = head[5];
    const double cutoff = par[0], alpha = par[1];
    if (N < 1 || C < 1 || T < 1 || seg < 1 || seg > DC_SEG_MAX || !dc_sizes_ok(H, W) || !(cutoff > 0) || !(alpha > 0)) fail("bad header");
    const size_t F = (size_t)N * C, cells = (size_t)H * W, n = F * cells;
    Arr<float> thr("thr", (size_t)T), y("y", n), p("p", n);
    if (std::fread(thr.v.data(), sizeof(float), (size_t)T, in) != (size_t)T || std::fread(y.v.data(), sizeof(float), n, in) != n ||
        std::fread(p.v.data(), sizeof(float), n, in) != n)
        fail("short case file");
    std::fclose(in);

    Arr<long long> counts("counts", F * T * DC_NCOUNT);
    Arr<double> sums("sums", F * T * DC_NSUM);
    Arr<int> d2_obs("d2_obs", F * T * cells), d2_pred("d2_pred", F * T * cells);
    const int nseg = dc_segments(W, seg);

    for (int t0 = 0; t0 < T; t0 += DC_TG) {                                // one chunk of all fields, groups of DC_TG thresholds
        const int tc = T - t0 < DC_TG ? T - t0 : DC_TG;
        Arr<uint16_t> g("g", F * (size_t)tc * 2 * cells, (uint16_t)7);
        Arr<long long> pc("row counts", F * (size_t)tc * H * DC_NCOUNT, -5);
        Arr<double> ps("row sums", F * (size_t)tc * H * DC_NSUM, -5.0);
        auto store = [&](int v) { return dc_g_pack(v); };
        auto fetch = [&](uint16_t v) { return dc_g_unpack(v); };
        // column pass: one lane per column, down and up again
        for (size_t f = 0; f < F; ++f)
            for (int j = 0; j < W; ++j) {
                int since[2][DC_TG];
                for (int k = 0; k < DC_TG; ++k) since[0][k] = since[1][k] = DC_G_NONE;
                for (int i = 0; i < H; ++i) {
                    const size_t o = dc_x_index(f, i, j, H, W, C);
                    const float yv = y.at(o), pv = p.at(o);
                    const bool ok = dc_valid(yv, pv);
                    for (int k = 0; k < tc; ++k) {
                        since[0][k] = dc_col_step(since[0][k], dc_event(ok, yv, thr.at((size_t)(t0 + k))));
                        since[1][k] = dc_col_step(since[1][k], dc_event(ok, pv, thr.at((size_t)(t0 + k))));
                        g.at(dc_g_index(f, tc, k, 0, H, W, i, j)) = store(since[0][k]);
                        g.at(dc_g_index(f, tc, k, 1, H, W, i, j)) = store(since[1][k]);
                    }
                }
                for (int k = 0; k < DC_TG; ++k) since[0][k] = since[1][k] = DC_G_NONE;
                for (int i = H - 1; i >= 0; --i)
                    for (int k = 0; k < tc; ++k)
                        for (int side = 0; side < 2; ++side) {
                            uint16_t& at = g.at(dc_g_index(f, tc, k, side, H, W, i, j));
                            const int down = fetch(at);
                            since[side][k] = dc_col_step(since[side][k], down == 0);
                            const int m = dc_col_join(down, since[side][k]);
                            if (m != down) at = store(m);
                        }
            }
        // row pass: one wave per (field, threshold, row)
        Arr<int> row2a("segment of side 0", (size_t)seg), row2b("segment of side 1", (size_t)seg);
        for (size_t f = 0; f < F; ++f)
            for (int k = 0; k < tc; ++k)
                for (int i = 0; i < H; ++i) {
                    std::vector<DcTerms> acc(LANES);
                    for (auto& a : acc) dc_zero(&a);
                    int staged = -1, mina = DC_DIST_EMPTY, minb = DC_DIST_EMPTY;
                    for (int j0 = 0; j0 < W; j0 += LANES) {
                        const int own = j0 / seg;
                        int da[LANES], db[LANES], jj[LANES];
                        bool inside[LANES];
                        for (int l = 0; l < LANES; ++l) {
                            inside[l] = j0 + l < W;
                            jj[l] = inside[l] ? j0 + l : W - 1;
                            da[l] = db[l] = DC_DIST_EMPTY;
                        }
                        for (int step = 0; step < 2 * nseg - 1; ++step) {
                            const int s = dc_seg_visit(own, step);
                            if (s < 0 || s >= nseg) continue;
                            const int a = s * seg, b = a + seg < W ? a + seg : W;
                            bool any = false;
                            for (int l = 0; l < LANES; ++l)
                                any = any || (inside[l] && dc_seg_needed(dc_seg_offset(jj[l], a, b), da[l] > db[l] ? da[l] : db[l]));
                            if (!any) continue;
                            if (staged != s) {
                                mina = minb = DC_DIST_EMPTY;
                                for (int c = 0; c < seg; ++c) row2a.at((size_t)c) = row2b.at((size_t)c) = -7;
                                for (int c = 0; c < b - a; ++c) {
                                    const int va = dc_g2(fetch(g.at(dc_g_index(f, tc, k, 0, H, W, i, a + c))));
                                    const int vb = dc_g2(fetch(g.at(dc_g_index(f, tc, k, 1, H, W, i, a + c))));
                                    row2a.at((size_t)c) = va; row2b.at((size_t)c) = vb;
                                    mina = va < mina ? va : mina; minb = vb < minb ? vb : minb;
                                }
                                staged = s;
                            }
                            for (int l = 0; l < LANES; ++l) {                // (a lane beyond the row repeats the last column's scan)
                                g_lo = row2a.v.data(); g_hi = g_lo + (b - a);
                                da[l] = dc_row_scan(row2a.v.data(), a, b, mina, jj[l], da[l]);
                                g_lo = row2b.v.data(); g_hi = g_lo + (b - a);
                                db[l] = dc_row_scan(row2b.v.data(), a, b, minb, jj[l], db[l]);
                            }
                        }
                        for (int l = 0; l < LANES; ++l) {
                            if (!inside[l]) continue;
                            const size_t o = dc_x_index(f, i, jj[l], H, W, C);
                            DcTerms t;
                            dc_cell_terms(dc_valid(y.at(o), p.at(o)), da[l], db[l], cutoff, alpha, &t);
                            dc_join(&acc[l], &t);
                            const size_t m = (dc_out_index(f, T, t0 + k) * (size_t)H + (size_t)i) * (size_t)W + (size_t)jj[l];
                            d2_obs.at(m) = da[l];
                            d2_pred.at(m) = db[l];
                        }
                    }
                    const DcTerms r = tree64(acc);
                    for (int q = 0; q < DC_NCOUNT; ++q) pc.at(dc_partial_index(f, tc, k, H, i, DC_NCOUNT) + q) = r.c[q];
                    for (int q = 0; q < DC_NSUM; ++q) ps.at(dc_partial_index(f, tc, k, H, i, DC_NSUM) + q) = r.s[q];
                }
        // final: thread t joins the rows t, t + 256, ...; a tree joins the threads
        for (size_t f = 0; f < F; ++f)
            for (int k = 0; k < tc; ++k) {
                std::vector<DcTerms> red(FINAL_THREADS);
                for (int t = 0; t < FINAL_THREADS; ++t) {
                    dc_zero(&red[t]);
                    for (int i = t; i < H; i += FINAL_THREADS) {
                        DcTerms r;
                        for (int q = 0; q < DC_NCOUNT; ++q) r.c[q] = pc.at(dc_partial_index(f, tc, k, H, i, DC_NCOUNT) + q);
                        for (int q = 0; q < DC_NSUM; ++q) r.s[q] = ps.at(dc_partial_index(f, tc, k, H, i, DC_NSUM) + q);
                        dc_join(&red[t], &r);
                    }
                }
                for (int o = FINAL_THREADS / 2; o > 0; o >>= 1)
                    for (int t = 0; t < o; ++t) dc_join(&red[t], &red[t + o]);
                for (int q = 0; q < DC_NCOUNT; ++q) counts.at(dc_out_index(f, T, t0 + k) * DC_NCOUNT + q) = red[0].c[q];
                for (int q = 0; q < DC_NSUM; ++q) sums.at(dc_out_index(f, T, t0 + k) * DC_NSUM + q) = red[0].s[q];
            }
    }
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) fail("cannot open the output file");
    counts.write(out); sums.write(out); d2_obs.write(out); d2_pred.write(out);
    if (std::fclose(out) != 0) std::exit(3);
    return 0;
}
