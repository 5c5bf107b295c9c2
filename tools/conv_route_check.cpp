// Prints what dl4ds_amd/csrc/conv_route.h decides for a list of calls: host code only, no device call, nothing is dereferenced.
//
//   hipcc -std=c++17 -x hip --offload-host-only -o conv_route_check tools/conv_route_check.cpp
//   (-DCONV_ROUTE_WITH_LIBRARY and linked with dl4ds_amd/libdl4ds_hip.so: also the `ws` lines)
//   conv_route_check calls.txt
//
// calls.txt, one call per line:
//   fwd   KS IN OUT ADD MASK POOL BIAS    -> fwd <family> <refusal | ->          (ADD / MASK: a view or -, POOL: 0 | 1,
//   wgrad KS X DZ                         -> wgrad <family> <slabs> <refusal | ->   BIAS: byte offset of the bias pointer or -)
//   ws    KS X DZ                         -> ws <conv2d_wgrad_workspace_bytes>
// a view: N,H,W,C,ld,d2s,off,aff -- ld floats per pixel (0: dense), d2s 0 | r, off: the base pointer's offset in floats from a
// 16-byte aligned address or n for a null pointer, aff: 0 plain | 1 scale | 2 scale and shift.  Views are built the way capi.cpp's
// desc_view builds them.  tests/test_conv_route.py holds the expected side.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "../dl4ds_amd/csrc/conv_route.h"

#ifdef CONV_ROUTE_WITH_LIBRARY
size_t conv2d_wgrad_workspace_bytes(const TView& x, const TView& dz, int KS);
#endif

static float* const kBase = reinterpret_cast<float*>(uintptr_t(1) << 20);          // (addresses only)
static const float* const kAffine = reinterpret_cast<const float*>(uintptr_t(2) << 20);

static TView parse_view(const std::string& tok) {
    int N, H, W, C, ld, d2s, aff;
    char off[32];
    if (std::sscanf(tok.c_str(), "%d,%d,%d,%d,%d,%d,%31[^,],%d", &N, &H, &W, &C, &ld, &d2s, off, &aff) != 8) {
        std::fprintf(stderr, "conv_route_check: bad view '%s'\n", tok.c_str());
        std::exit(2);
    }
    float* p = off[0] == 'n' ? nullptr : kBase + std::atoi(off);
    TView v;
    if (d2s > 1) {
        v = make_view_d2s(p, N, H, W, C, d2s);
        if (ld) { v.ld = ld; v.vec = v.vec && (ld & 3) == 0; }
    } else {
        v = make_pitched_view(p, N, H, W, C, ld ? ld : C, (size_t)H * W * (ld ? ld : C));
    }
    if (aff >= 1) v.sc = kAffine;
    if (aff >= 2) v.sh = kAffine + 4096;
    return v;
}

static const char* name_of(ConvFwdFamily f) {
    switch (f) {
        case ConvFwdFamily::Direct: return "Direct";
        case ConvFwdFamily::NarrowPair: return "NarrowPair";
        case ConvFwdFamily::Narrow: return "Narrow";
        case ConvFwdFamily::Pointwise: return "Pointwise";
        default: return "Rest";
    }
}
static const char* name_of(WgradFamily f) {
    switch (f) {
        case WgradFamily::Direct: return "Direct";
        case WgradFamily::Narrow: return "Narrow";
        case WgradFamily::NarrowSlices: return "NarrowSlices";
        default: return "General";
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: conv_route_check calls.txt\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string what, a, b;
        int KS;
        if (!(ss >> what >> KS >> a >> b)) continue;
        if (what == "fwd") {
            std::string add, mask, bias;
            int pool;
            if (!(ss >> add >> mask >> pool >> bias)) { std::fprintf(stderr, "conv_route_check: bad line '%s'\n", line.c_str()); return 2; }
            ConvEpilogue ep;
            if (add != "-") ep.add = parse_view(add);
            if (mask != "-") ep.mask = parse_view(mask);
            if (pool) ep.pool = kBase;
            if (bias != "-") ep.bias = reinterpret_cast<const float*>(reinterpret_cast<const char*>(kBase) + std::atoi(bias.c_str()));
            const ConvFwdRoute r = conv2d_forward_route(parse_view(a), parse_view(b), KS, ep);
            std::printf("fwd %s %s\n", name_of(r.family), r.refusal ? r.refusal : "-");
        } else if (what == "wgrad") {
            const WgradRoute r = conv2d_wgrad_route(parse_view(a), parse_view(b), KS);
            std::printf("wgrad %s %d %s\n", name_of(r.family), r.slabs, r.refusal ? r.refusal : "-");
#ifdef CONV_ROUTE_WITH_LIBRARY
        } else if (what == "ws") {
            std::printf("ws %zu\n", conv2d_wgrad_workspace_bytes(parse_view(a), parse_view(b), KS));
#endif
        } else {
            std::fprintf(stderr, "conv_route_check: bad line '%s'\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
