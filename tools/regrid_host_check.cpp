// The regridding of dl4ds_amd/csrc/regrid.hip, run on the CPU: the same decomposition (a workgroup per slab of one output row, the
// x-taps of its columns staged or read in place, a lane per element or per four channels) and the same summation order of the
// consistency sums (a lane's cells ascending, the tree over 256 lanes, the rows ascending) through the functions of regrid_core.h,
// with every array access checked.  A stray index prints the array and the index and ends the program with status 2.
//
//   c++ -std=c++17 -O1 -ffp-contract=off -o regrid_host_check tools/regrid_host_check.cpp
//                                                                   (sanitizers: add -fsanitize=address,undefined -fno-sanitize-recover=all)
//   regrid_host_check case.bin out.bin
//
// case.bin: int32 N, H, W, C, H', W', skipna, V (1: the 4-byte form, 4: the 16-byte form, C % 4 == 0), nnz_y, nnz_x; fp64 min_valid;
//           int32 yptr[H' + 1], yidx[nnz_y], xptr[W' + 1], xidx[nnz_x]; fp64 yw[nnz_y], xw[nnz_x], ay[H'], ax[W'];
//           float32 x[N][H][W][C], ref[N][H'][W'][C].
// out.bin:  float32 out[N][H'][W'][C], fp64 sums[N][C][6], int64 counts[N][C][2], float32 resid[N][H'][W'][C].
// tests/test_regrid_device_api.py compares that with tests/regrid_ref.py on every case of tests/regrid_cases.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

static const float* g_lo = nullptr;
static const float* g_hi = nullptr;
static void check_x(const float* p, int n) {
    if (p < g_lo || p + n > g_hi) {
        std::fprintf(stderr, "regrid_host_check: x[%lld .. +%d) is outside [0, %lld)\n", (long long)(p - g_lo), n, (long long)(g_hi - g_lo));
        std::exit(2);
    }
}
#define RG_CHECK_X(p, n) check_x(p, n)
#include "../dl4ds_amd/csrc/regrid_core.h"

static void fail(const char* what) { std::fprintf(stderr, "regrid_host_check: %s\n", what); std::exit(1); }

template <typename T>
struct Arr {
    std::vector<T> v;
    const char* name;
    Arr(const char* n, size_t size, T fill = T()) : v(size, fill), name(n) {}
    T& at(size_t k) {
        if (k >= v.size()) {
            std::fprintf(stderr, "regrid_host_check: %s[%zu] is outside [0, %zu)\n", name, k, v.size());
            std::exit(2);
        }
        return v[k];
    }
    void read(std::FILE* f) { if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) fail("short case file"); }
    void write(std::FILE* f) { if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3); }
};
// a table the walk indexes: every access checked against the taps the owner may read
template <typename T>
struct View {
    Arr<T>* a;
    size_t base, count;
    T operator[](int k) const {
        if (k < 0 || (size_t)k >= count) {
            std::fprintf(stderr, "regrid_host_check: tap %d of %s is outside [0, %zu)\n", k, a->name, count);
            std::exit(2);
        }
        return a->at(base + (size_t)k);
    }
};

struct Tables {
    Arr<int> yptr, yidx, xptr, xidx;
    Arr<double> yw, xw, ay, ax;
};

template <int V>
static void cell(Tables& t, View<int> ix, View<double> wx, int p0, const float* xs, int W, int C, int i, int j, int c, bool skipna,
                 double min_valid, float* r) {
    RgAcc acc[V];
    const int ya = t.yptr.at((size_t)i), yb = t.yptr.at((size_t)i + 1);
    const int xa = t.xptr.at((size_t)j), xb = t.xptr.at((size_t)j + 1);
    for (int a = ya; a < yb; ++a) (void)t.yidx.at((size_t)a);              // (the walk reads them through plain pointers)
    rg_walk<V>(xs, W, C, t.yidx.v.data(), t.yw.v.data(), ya, yb, ix, wx, xa - p0, xb - p0, c, skipna, acc);
    for (int k = 0; k < V; ++k) r[k] = rg_finish(acc + k, min_valid);
}

// the x-taps of the columns [j0, j1): a staged copy when they fit (what the kernel keeps in LDS), the table itself otherwise
struct Stage {
    Arr<int> idx{"staged xidx", RG_LDS_TAPS, -7};
    Arr<double> w{"staged xw", RG_LDS_TAPS, -7.0};
    View<int> vi;
    View<double> vw;
    int p0;
    void fill(Tables& t, int j0, int j1) {
        p0 = t.xptr.at((size_t)j0);
        const int p1 = t.xptr.at((size_t)j1);
        if (rg_taps_in_lds(p1 - p0)) {
            for (int k = 0; k < p1 - p0; ++k) { idx.at((size_t)k) = t.xidx.at((size_t)(p0 + k)); w.at((size_t)k) = t.xw.at((size_t)(p0 + k)); }
            vi = View<int>{&idx, 0, (size_t)(p1 - p0)};
            vw = View<double>{&w, 0, (size_t)(p1 - p0)};
        } else {
            vi = View<int>{&t.xidx, (size_t)p0, (size_t)(p1 - p0)};
            vw = View<double>{&t.xw, (size_t)p0, (size_t)(p1 - p0)};
        }
    }
};

template <int V>
static void apply(Tables& t, Arr<float>& x, Arr<float>& out, int N, int H, int W, int C, int Ho, int Wo, bool skipna, double min_valid) {
    const rg_i64 row = (rg_i64)Wo * C;
    const int nb = rg_row_blocks(row, V);
    Stage st;
    for (int n = 0; n < N; ++n)
        for (int i = 0; i < Ho; ++i)
            for (int b = 0; b < nb; ++b) {
                int j0, j1;
                rg_block_cols(b, V, Wo, C, &j0, &j1);
                st.fill(t, j0, j1);
                for (int lane = 0; lane < RG_THREADS; ++lane) {
                    const rg_i64 e = ((rg_i64)b * RG_THREADS + lane) * V;
                    if (e >= row) continue;
                    const int j = (int)(e / C), c = (int)(e - (rg_i64)j * C);
                    if (j < j0 || j >= j1) fail("a lane's column lies outside its workgroup's columns");
                    const float* xs = x.v.data() + (size_t)n * H * W * C;
                    float r[V];
                    cell<V>(t, st.vi, st.vw, st.p0, xs, W, C, i, j, c, skipna, min_valid, r);
                    for (int k = 0; k < V; ++k) out.at(rg_index((size_t)n, i, j, c + k, Ho, Wo, C)) = r[k];
                }
            }
}

int main(int argc, char** argv) {
    if (argc != 3) fail("usage: regrid_host_check case.bin out.bin");
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) fail("cannot open the case file");
    int head[10];
    double min_valid;
    if (std::fread(head, sizeof(int), 10, in) != 10 || std::fread(&min_valid, sizeof(double), 1, in) != 1) fail("short header");
    const int N = head[0], H = head[1], W = head[2], C = head[3], Ho = head[4], Wo = head[5], V = head[7], ny = head[8], nx = head[9];
    const bool skipna = head[6] != 0;
    if (N < 1 || C < 1 || !rg_sizes_ok(H, W) || !rg_sizes_ok(Ho, Wo) || ny < 0 || nx < 0 || !(min_valid >= 0.0 && min_valid <= 1.0) ||
        !(V == 1 || (V == RG_VEC && C % RG_VEC == 0)))
        fail("bad header");
    Tables t{Arr<int>("yptr", (size_t)Ho + 1), Arr<int>("yidx", (size_t)ny), Arr<int>("xptr", (size_t)Wo + 1), Arr<int>("xidx", (size_t)nx),
             Arr<double>("yw", (size_t)ny), Arr<double>("xw", (size_t)nx), Arr<double>("ay", (size_t)Ho), Arr<double>("ax", (size_t)Wo)};
    t.yptr.read(in); t.yidx.read(in); t.xptr.read(in); t.xidx.read(in); t.yw.read(in); t.xw.read(in); t.ay.read(in); t.ax.read(in);
    const size_t n_in = (size_t)N * H * W * C, n_out = (size_t)N * Ho * Wo * C;
    Arr<float> x("x", n_in), ref("ref", n_out);
    x.read(in); ref.read(in);
    std::fclose(in);
    if (t.yptr.at(0) != 0 || t.xptr.at(0) != 0 || t.yptr.at((size_t)Ho) != ny || t.xptr.at((size_t)Wo) != nx) fail("bad ptr");
    for (int k = 0; k < ny; ++k) if (t.yidx.at((size_t)k) < 0 || t.yidx.at((size_t)k) >= H) fail("bad yidx");
    for (int k = 0; k < nx; ++k) if (t.xidx.at((size_t)k) < 0 || t.xidx.at((size_t)k) >= W) fail("bad xidx");
    g_lo = x.v.data(); g_hi = g_lo + n_in;

    Arr<float> out("out", n_out, -5.f), resid("resid", n_out, -5.f);
    if (V == RG_VEC) apply<RG_VEC>(t, x, out, N, H, W, C, Ho, Wo, skipna, min_valid);
    else apply<1>(t, x, out, N, H, W, C, Ho, Wo, skipna, min_valid);

    // consistency: a workgroup per (n, i'), the whole row's x-taps staged; one channel at a time
    Arr<double> part_s("row sums", (size_t)N * C * Ho * RG_NSUM, -5.0), sums("sums", (size_t)N * C * RG_NSUM);
    Arr<rg_i64> part_c("row counts", (size_t)N * C * Ho * RG_NCOUNT, -5), counts("counts", (size_t)N * C * RG_NCOUNT);
    Stage st;
    st.fill(t, 0, Wo);
    for (int n = 0; n < N; ++n)
        for (int i = 0; i < Ho; ++i)
            for (int c = 0; c < C; ++c) {
                std::vector<RgCons> red(RG_THREADS);
                for (int lane = 0; lane < RG_THREADS; ++lane) {
                    rg_cons_zero(&red[lane]);
                    for (int j = lane; j < Wo; j += RG_THREADS) {
                        float r;
                        cell<1>(t, st.vi, st.vw, st.p0, x.v.data() + (size_t)n * H * W * C, W, C, i, j, c, skipna, min_valid, &r);
                        const size_t o = rg_index((size_t)n, i, j, c, Ho, Wo, C);
                        if (r != out.at(o) && !(r != r && out.at(o) != out.at(o))) fail("consistency and apply disagree on a value");
                        resid.at(o) = rg_cons_cell(&red[lane], r, ref.at(o), rg_area(t.ay.at((size_t)i), t.ax.at((size_t)j)));
                    }
                }
                for (int o = RG_THREADS / 2; o > 0; o >>= 1)
                    for (int lane = 0; lane < o; ++lane) rg_cons_join(&red[lane], &red[lane + o]);
                for (int k = 0; k < RG_NSUM; ++k) part_s.at(rg_partial_index((size_t)n, c, i, C, Ho, RG_NSUM) + k) = red[0].s[k];
                for (int k = 0; k < RG_NCOUNT; ++k) part_c.at(rg_partial_index((size_t)n, c, i, C, Ho, RG_NCOUNT) + k) = red[0].c[k];
            }
    for (size_t f = 0; f < (size_t)N * C; ++f) {
        RgCons acc;
        rg_cons_zero(&acc);
        for (int i = 0; i < Ho; ++i) {
            RgCons r;
            for (int k = 0; k < RG_NSUM; ++k) r.s[k] = part_s.at((f * Ho + i) * RG_NSUM + k);
            for (int k = 0; k < RG_NCOUNT; ++k) r.c[k] = part_c.at((f * Ho + i) * RG_NCOUNT + k);
            rg_cons_join(&acc, &r);
        }
        for (int k = 0; k < RG_NSUM; ++k) sums.at(f * RG_NSUM + k) = acc.s[k];
        for (int k = 0; k < RG_NCOUNT; ++k) counts.at(f * RG_NCOUNT + k) = acc.c[k];
    }
    std::FILE* of = std::fopen(argv[2], "wb");
    if (!of) fail("cannot open the output file");
    out.write(of); sums.write(of); counts.write(of); resid.write(of);
    if (std::fclose(of) != 0) std::exit(3);
    return 0;
}
