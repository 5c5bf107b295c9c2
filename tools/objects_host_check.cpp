// The object labelling of dl4ds_amd/csrc/objects.hip, run on the CPU: the same five steps (init, merge, flatten, number, gather)
// unit by unit and cell by cell through the functions of objects_core.h, with every array access checked.  A stray index prints
// the array and the index and ends the program with status 2.
//
//   c++ -std=c++17 -O1 -o objects_host_check tools/objects_host_check.cpp         (sanitizers: add -fsanitize=address,undefined)
//   objects_host_check case.bin out.bin
//
// case.bin: int32 N, H, W, C, connectivity, cap (-1: the largest count), then float32 thr[N*C], then float32 x[N][H][W][C].
// out.bin:  int32 cap, then labels int32 [F][H][W], count int32 [F], nvalid int64 [F], field_sums fp64 [F][3], sums int64
//           [F][cap][6], bbox int32 [F][cap][4], first int32 [F][cap], vmax float32 [F][cap], mass fp64 [F][cap][3].
// tests/test_objects_device_api.py compares that with tests/objects_ref.py on every case of tests/objects_cases.py.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static const int* g_lo = nullptr;
static const int* g_hi = nullptr;
static const char* g_name = "";
static void check_access(const int* p) {
    if (p < g_lo || p >= g_hi) {
        std::fprintf(stderr, "objects_host_check: %s[%lld] is outside [0, %lld)\n", g_name, (long long)(p - g_lo), (long long)(g_hi - g_lo));
        std::exit(2);
    }
}
#define OC_CHECK_ACCESS(p) check_access(p)
#include "../dl4ds_amd/csrc/objects_core.h"

template <typename T>
struct Arr {
    std::vector<T> v;
    const char* name;
    Arr(const char* n, size_t size, T fill = T()) : v(size, fill), name(n) {}
    T& at(long long k) {
        if (k < 0 || (size_t)k >= v.size()) {
            std::fprintf(stderr, "objects_host_check: %s[%lld] is outside [0, %zu)\n", name, k, v.size());
            std::exit(2);
        }
        return v[(size_t)k];
    }
    void write(std::FILE* f) { if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3); }
};
// the int array that the walks of objects_core.h may touch from here on
static void watch(Arr<int>& a, size_t from, size_t n) {
    g_lo = a.v.data() + from; g_hi = g_lo + n; g_name = a.name;
}
static void fail(const char* what) { std::fprintf(stderr, "objects_host_check: %s\n", what); std::exit(1); }

int main(int argc, char** argv) {
    if (argc != 3) fail("usage: objects_host_check case.bin out.bin");
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) fail("cannot open the case file");
    int head[6];
    if (std::fread(head, sizeof(int), 6, in) != 6) fail("short header");
    const int N = head[0], H = head[1], W = head[2], C = head[3], connectivity = head[4];
    int cap = head[5];
    if (N < 1 || H < 1 || W < 1 || C < 1 || (connectivity != 1 && connectivity != 2) || cap < -1) fail("bad header");
    const size_t F = (size_t)N * C, cells = (size_t)H * W;
    const oc_i64 units = oc_units(H, W);
    Arr<float> thr("thr", F), x("x", F * cells);
    if (std::fread(thr.v.data(), sizeof(float), F, in) != F || std::fread(x.v.data(), sizeof(float), F * cells, in) != F * cells)
        fail("short case file");
    std::fclose(in);

    Arr<int> parent("parent", F * cells), rootlabel("rootlabel", F * cells, -7), ucount("ucount", F * (size_t)units);
    Arr<int> labels("labels", F * cells), count("count", F);
    Arr<long long> nvalid("nvalid", F);
    Arr<double> field_sums("field_sums", F * 3);
    auto xat = [&](size_t f, int i, int j) -> float { return x.at((long long)oc_x_index(f, i, j, H, W, C)); };

    for (size_t f = 0; f < F; ++f) {
        const long long off = (long long)(f * cells);
        // init
        for (oc_i64 u = 0; u < units; ++u) {
            int i, j0;
            oc_unit_pos(u, W, &i, &j0);
            uint64_t mask = 0;
            for (int lane = 0; lane < OC_SEG && j0 + lane < W; ++lane) {
                const float v = xat(f, i, j0 + lane);
                if (oc_event(v, thr.at((long long)f))) mask |= 1ull << lane;
                if (oc_finite(v)) {
                    nvalid.at((long long)f) += 1;
                    field_sums.at(3 * (long long)f) += (double)v;
                    field_sums.at(3 * (long long)f + 1) += (double)v * i;
                    field_sums.at(3 * (long long)f + 2) += (double)v * (j0 + lane);
                }
            }
            for (int lane = 0; lane < OC_SEG && j0 + lane < W; ++lane)
                parent.at(off + oc_cell(i, j0 + lane, W)) = oc_init_parent(mask, lane, i, j0, W);
        }
        // merge, flatten
        watch(parent, f * cells, cells);
        // (the cells in a scattered order, k -> k * p mod cells with a prime p that does not divide cells: the device has no order
        // either, and the outcome must not depend on it)
        const unsigned long long primes[3] = {7919, 104729, 1299709};
        unsigned long long p = 1;
        for (int k = 0; k < 3 && p == 1; ++k)
            if (cells % primes[k]) p = primes[k];
        for (unsigned long long k = 0; k < cells; ++k) {
            const unsigned long long idx = k * p % cells;
            if (!oc_merge_cell(parent.v.data() + off, H, W, connectivity, (int)(idx / W), (int)(idx % W))) fail("a union passed its bound");
        }
        for (oc_i64 u = 0; u < units; ++u) {
            int i, j0, n = 0;
            oc_unit_pos(u, W, &i, &j0);
            for (int lane = 0; lane < OC_SEG && j0 + lane < W; ++lane) {
                const int idx = oc_cell(i, j0 + lane, W);
                const int r = oc_root(parent.v.data() + off, (int)cells, idx);
                if (r == -2) fail("a walk passed its bound");
                if (r >= 0) parent.at(off + idx) = r;
                n += r == idx;
            }
            ucount.at((long long)f * units + u) = n;
        }
        // number: exclusive scan of the units' root counts, then the roots' labels
        int running = 0;
        for (oc_i64 u = 0; u < units; ++u) {
            const int c = ucount.at((long long)f * units + u);
            ucount.at((long long)f * units + u) = running;
            running += c;
        }
        count.at((long long)f) = running;
        for (oc_i64 u = 0; u < units; ++u) {
            int i, j0, rank = 0;
            oc_unit_pos(u, W, &i, &j0);
            for (int lane = 0; lane < OC_SEG && j0 + lane < W; ++lane) {
                const int idx = oc_cell(i, j0 + lane, W);
                if (parent.at(off + idx) == idx) rootlabel.at(off + idx) = ucount.at((long long)f * units + u) + rank++ + 1;
            }
        }
    }
    if (cap < 0) {
        cap = 0;
        for (size_t f = 0; f < F; ++f) cap = count.at((long long)f) > cap ? count.at((long long)f) : cap;
    }
    const size_t rows = F * (size_t)cap;
    Arr<long long> sums("sums", rows * 6);
    Arr<int> bbox("bbox", rows * 4), first("first", rows);
    Arr<unsigned> vkey("vmax", rows);
    Arr<double> mass("mass", rows * 3);
    for (size_t r = 0; r < rows; ++r) {
        bbox.at(4 * (long long)r) = bbox.at(4 * (long long)r + 2) = INT_MAX;
        bbox.at(4 * (long long)r + 1) = bbox.at(4 * (long long)r + 3) = INT_MIN;
    }
    // gather: one set of table updates per run of consecutive event lanes
    for (size_t f = 0; f < F; ++f) {
        const long long off = (long long)(f * cells);
        watch(rootlabel, f * cells, cells);
        for (oc_i64 u = 0; u < units; ++u) {
            int i, j0, lab[OC_SEG] = {};
            oc_unit_pos(u, W, &i, &j0);
            uint64_t mask = 0;
            for (int lane = 0; lane < OC_SEG && j0 + lane < W; ++lane) {
                const int idx = oc_cell(i, j0 + lane, W);
                lab[lane] = oc_label(rootlabel.v.data() + off, (int)cells, parent.at(off + idx));
                if (lab[lane] < 0) fail("a root outside the field");
                labels.at(off + idx) = lab[lane];
                if (lab[lane] > 0) mask |= 1ull << lane;
            }
            for (int lane = 0; lane < OC_SEG && j0 + lane < W; ++lane) {
                if (!lab[lane]) continue;
                const oc_i64 row = oc_table_row(f, lab[lane], cap);
                if (row < 0) continue;
                const int j = j0 + lane, idx = oc_cell(i, j, W);
                if (parent.at(off + idx) == idx) first.at(row) = idx;
                if (oc_run_first(mask, lane) != lane) continue;
                const int len = oc_run_len(mask, lane);
                oc_i64 s[6];
                oc_run_sums(i, j, len, s);
                for (int k = 0; k < 6; ++k) sums.at(6 * row + k) += s[k];
                if (i < bbox.at(4 * row)) bbox.at(4 * row) = i;
                if (i > bbox.at(4 * row + 1)) bbox.at(4 * row + 1) = i;
                if (j < bbox.at(4 * row + 2)) bbox.at(4 * row + 2) = j;
                if (j + len - 1 > bbox.at(4 * row + 3)) bbox.at(4 * row + 3) = j + len - 1;
                for (int k = 0; k < len; ++k) {
                    if (lab[lane + k] != lab[lane]) fail("two labels in one run");
                    const float v = xat(f, i, j + k);
                    if (oc_key(v) > vkey.at(row)) vkey.at(row) = oc_key(v);
                    mass.at(3 * row) += (double)v;
                    mass.at(3 * row + 1) += (double)v * i;
                    mass.at(3 * row + 2) += (double)v * (j + k);
                }
            }
        }
    }
    // finish
    for (size_t r = 0; r < rows; ++r) {
        if ((int)(r % (size_t)cap) < count.at((long long)(r / (size_t)cap))) {
            vkey.at((long long)r) = oc_bits(oc_unkey(vkey.at((long long)r)));
        } else {
            vkey.at((long long)r) = 0u;
            for (int k = 0; k < 4; ++k) bbox.at(4 * (long long)r + k) = 0;
        }
    }
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) fail("cannot open the output file");
    if (std::fwrite(&cap, sizeof(int), 1, out) != 1) std::exit(3);
    labels.write(out); count.write(out); nvalid.write(out); field_sums.write(out);
    sums.write(out); bbox.write(out); first.write(out); vkey.write(out); mass.write(out);
    if (std::fclose(out) != 0) std::exit(3);
    return 0;
}
