// dl4ds_amd -- 1x1 convolutions with float4-able channel counts (Cin, Cout multiples of 4, up to 48) as a plain HBM stream.
//
// Replaces (for those shapes) tf.keras.layers.Conv2D(kernel_size=1) forward and its Conv2DBackpropInput -- the projected skips of
// the residual blocks (dl4ds/models/blocks.py:208) and TransitionSkip / TransitionBlock (blocks.py:299) -- which used to run on
// conv_stream_ws_kernel<1,..>: 16 x 16-pixel tiles staged through LDS by helper waves, built for the halos of 3x3 / 5x5 layers.
//
// A 1x1 layer is a GEMM [pixels x Cin] x [Cin x Cout] over the FLATTENED pixels of an NHWC view (pixel pitch ld >= C, images
// contiguous): no halo, so nothing has to meet in LDS.  Per wave and 16 pixels:
//   * lane (l15, lq) loads channels [KT lq, KT lq + KT) of pixel l15 (KT = Cin / 4) with buffer loads straight into the second MFMA
//     operand: in the e-th v_mfma_f32_16x16x4_f32 k-slot q carries channel KT q + e -- the assignment of conv_stream_kernel and
//     conv_stream_ws_kernel (their E = Cin / 4).  With fewer than 16 input channels, which ran on conv_igemm_kernel, k-slot q carries
//     channel 4 e + q as there.  The bias starts the accumulators where conv_stream_ws_kernel would have run and is added last
//     otherwise (stream_ws_order below).  So every output keeps the order of its sum, and with it its bits, on every layer those
//     kernels took with Cin / 4 even or under 4; only conv_igemm's small grids (< 256 pixels per image) with 16 and more channels and
//     the odd chunk widths (Cin = 20, 28, 36, 44: padded chunks there) are rounded differently.  (With k-slot q = channel 4 q + e
//     inside 16-channel groups, as conv_narrow_pair_ws<.., C16> reads its tiles, a 24- or 40-channel input would need masked loads
//     beyond its channels and no layer above 16 channels would keep its bits.)
//   * the filter (<= 48 x 48, zero beyond Cout) is the FIRST operand, KT x NT registers loaded once per wave: D[cout][pixel], so a lane
//     ends up with four CONSECUTIVE output channels of one pixel and stores them as one float4 -- no transpose, no LDS, no barrier,
//     zero instructions per MFMA between the accumulators and the store (the alternative, pixels on the rows, needs an LDS round trip
//     of 2 NT instructions per KT NT MFMAs).
//   * the descriptors end with the last pixel of the view: pixels beyond it load zeros and their stores are dropped.
// A wave walks blocks of MB x 16 pixels with a grid stride; the next block's loads are issued before the current block's MFMAs.
// Registers (gfx950, from the compile; part of the filter lives in accumulation registers, no scratch anywhere): the forms without
// an epilogue operand take 32-122 vector + 8-48 accumulation registers = 3-8 waves per SIMD (40 -> 48 with a bias: 102 + 36, 3 waves),
// the forms with one operand 48-152 + 8-48 = 2-8 (48 -> 40 with a mask: 142 + 36, 2 waves), mask + accumulate 57-188 + 8-38 = 2-7.
// The grid is what is resident at that occupancy (resident_blocks): a wave walks 8-32 blocks at 64 x 128^2.  Measured there:
// 3.9-6.8 TB/s per launch (profiles/bench_breakdown_pointwise.json); the three-cout-tile forms at 2-3 waves are the slowest.
#include "ops.h"
#include "conv_route.h"
#include "launch.h"
#include "prof.h"
#include <algorithm>
#include <cstdlib>
#include <string>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int PW_OOB = (int)0xffffff00u;         // beyond every descriptor's record count: loads return 0, stores are dropped
constexpr int PW_RSRC3 = 0x00020000;             // gfx9 raw buffer, 32-bit data
constexpr int PW_ADD = 1, PW_RELU = 2, PW_MASK = 4, PW_ACC = 8;

struct PointwiseParams {
    const float* x; float* y;
    const float* add; const float* mask;
    const float* w; const float* bias;
    long long npx;                               // pixels of the flattened view
    int Cin, Cout;
    int ldx, ldy, lda, ldm;                      // pixel pitches in floats
    int bias_first;                              // the accumulators start at the bias (conv_stream_ws_kernel's order) / it is added last
};

// bytes from pixel p0 of a view to the end of its last pixel, as a descriptor's record count
__device__ __forceinline__ int pw_records(long long npx, long long p0, int ld, int C) {
    const long long b = ((npx - 1 - p0) * ld + C) * 4;
    return (int)(b < 0x7fffff00ll ? b : 0x7fffff00ll);
}

template <int KT>
__device__ __forceinline__ void pw_load(float (&dst)[KT], __amdgpu_buffer_rsrc_t rs, int off) {
    if constexpr (KT < 4) {                      // ascending assignment: channel 4 e + lq, 16 bytes apart
#pragma unroll
        for (int i = 0; i < KT; ++i) dst[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off + 16 * i, 0, 0));
    } else if constexpr (KT % 4 == 0) {
#pragma unroll
        for (int i = 0; i < KT / 4; ++i) {
            // (the whole vector is cast: __builtin_bit_cast of ONE element of an ext_vector reads element 0 whatever the index)
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16 * i, 0, 0));
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[4 * i + j] = v[j];
        }
    } else if constexpr (KT % 2 == 0) {          // Cin = 8, 24, 40: a lane's channels start on an 8-byte boundary
#pragma unroll
        for (int i = 0; i < KT / 2; ++i) {
            const f32x2 v = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, off + 8 * i, 0, 0));
            dst[2 * i] = v[0];
            dst[2 * i + 1] = v[1];
        }
    } else {
#pragma unroll
        for (int i = 0; i < KT; ++i) dst[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4 * i, 0, 0));
    }
}

// KT: k-steps = Cin / 4; NT: tiles of 16 output channels; EPI: PW_* bits (a null bias adds 0)
template <int KT, int NT, int EPI>
__global__ void __launch_bounds__(256) conv_pointwise_kernel(const PointwiseParams a) {
    constexpr int MB = KT <= 4 ? 4 : 2;          // 16-pixel groups per wave and step: 64 / 32 pixels in flight
    constexpr int PXW = 16 * MB;
    constexpr bool ADD = (EPI & PW_ADD) != 0, RELU = (EPI & PW_RELU) != 0, MASK = (EPI & PW_MASK) != 0, ACC = (EPI & PW_ACC) != 0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int Cin = a.Cin, Cout = a.Cout;

    // which channel k-slot lq carries in step e.  Fewer than 16 input channels: 4 e + lq, conv_igemm_kernel's assignment (the kernel
    // these layers ran on; one dword per lane and step, 16-byte runs per pixel).  Otherwise KT lq + e, conv_stream*'s.
    constexpr bool ASC = KT < 4;
    // filter fragments: first MFMA operand = W^T[cout = 16 t + l15][k-slot lq] of step e, zero beyond Cout
    float wr[NT][KT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < KT; ++e) {
            const int co = 16 * t + l15;
            const float v = a.w[(size_t)(ASC ? 4 * e + lq : KT * lq + e) * Cout + (co < Cout ? co : 0)];
            wr[t][e] = co < Cout ? v : 0.f;
        }
    // the bias: lane (pixel l15, rows 4 lq + r) owns couts 16 t + 4 lq + [0, 4).  Where conv_stream_ws_kernel would have taken the
    // layer (bias_first, decided by the launcher) the accumulators start at it, as there; otherwise it is added to the finished sum, as
    // conv_stream_kernel and conv_igemm_kernel do -- the two orders differ in the last bits, and results stay what they were
    f32x4 b0[NT];
    bool cok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int co = 16 * t + 4 * lq;
        cok[t] = co < Cout;
        b0[t] = (a.bias && cok[t]) ? *reinterpret_cast<const f32x4*>(a.bias + co) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // per-lane byte offsets inside a block (the same in every block)
    int xoff[MB], yoff[MB][NT], aoff[ADD ? MB : 1][NT], moff[MASK ? MB : 1][NT];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int px = 16 * m + l15;
        xoff[m] = (px * a.ldx + (ASC ? lq : KT * lq)) * 4;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int co = 16 * t + 4 * lq;
            yoff[m][t] = cok[t] ? (px * a.ldy + co) * 4 : PW_OOB;
            if (ADD) aoff[m][t] = cok[t] ? (px * a.lda + co) * 4 : PW_OOB;
            if (MASK) moff[m][t] = cok[t] ? (px * a.ldm + co) * 4 : PW_OOB;
        }
    }
    (void)Cin;
    const bool bias_first = a.bias_first != 0;
    const long long nblk = (a.npx + PXW - 1) / PXW;
    const long long first = (long long)blockIdx.x * 4 + wave, stride = (long long)gridDim.x * 4;
    auto rsrc = [&](const float* base, long long blk, int ld, int C) __attribute__((always_inline)) {
        const long long p0 = blk * PXW;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(base + p0 * ld)), 0,
                                                 pw_records(a.npx, p0, ld, C), PW_RSRC3);
    };
    float xc[MB][KT];
    if (first < nblk) {
        const __amdgpu_buffer_rsrc_t rx = rsrc(a.x, first, a.ldx, a.Cin);
#pragma unroll
        for (int m = 0; m < MB; ++m) pw_load<KT>(xc[m], rx, xoff[m]);
    }
    for (long long blk = first; blk < nblk; blk += stride) {
        const __amdgpu_buffer_rsrc_t ry = rsrc(a.y, blk, a.ldy, Cout);
        // what the epilogue reads of this block, then the next block's pixels: both in flight during the MFMAs
        i32x4_t ad[ADD ? MB : 1][NT], mk[MASK ? MB : 1][NT], old[ACC ? MB : 1][NT];
        if (ADD) {
            const __amdgpu_buffer_rsrc_t ra = rsrc(a.add, blk, a.lda, Cout);
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) ad[m][t] = __builtin_amdgcn_raw_buffer_load_b128(ra, aoff[m][t], 0, 0);
        }
        if (MASK) {
            const __amdgpu_buffer_rsrc_t rm = rsrc(a.mask, blk, a.ldm, Cout);
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) mk[m][t] = __builtin_amdgcn_raw_buffer_load_b128(rm, moff[m][t], 0, 0);
        }
        if (ACC) {
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) old[m][t] = __builtin_amdgcn_raw_buffer_load_b128(ry, yoff[m][t], 0, 0);
        }
        float xn[MB][KT];
        const long long nb = blk + stride;
        if (nb < nblk) {
            const __amdgpu_buffer_rsrc_t rx = rsrc(a.x, nb, a.ldx, a.Cin);
#pragma unroll
            for (int m = 0; m < MB; ++m) pw_load<KT>(xn[m], rx, xoff[m]);
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            f32x4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = bias_first ? b0[t] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < KT; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[t][e], xc[m][e], acc[t], 0, 0, 0);   // D[cout][pixel]
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                f32x4 r4 = acc[t];
                if (!bias_first) r4 += b0[t];
                if (ADD) r4 += __builtin_bit_cast(f32x4, ad[m][t]);
                if (RELU) { r4[0] = fmaxf(r4[0], 0.f); r4[1] = fmaxf(r4[1], 0.f); r4[2] = fmaxf(r4[2], 0.f); r4[3] = fmaxf(r4[3], 0.f); }
                if (MASK) {
                    const f32x4 mv = __builtin_bit_cast(f32x4, mk[m][t]);
                    r4[0] = mv[0] > 0.f ? r4[0] : 0.f; r4[1] = mv[1] > 0.f ? r4[1] : 0.f;
                    r4[2] = mv[2] > 0.f ? r4[2] : 0.f; r4[3] = mv[3] > 0.f ? r4[3] : 0.f;
                }
                if (ACC) r4 += __builtin_bit_cast(f32x4, old[m][t]);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4_t, r4), ry, yoff[m][t], 0, 0);
            }
        }
        if (nb < nblk) {
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int e = 0; e < KT; ++e) xc[m][e] = xn[m][e];
        }
    }
}

int pw_cu_count() {
    static const int n = [] {
        int dev = 0, v = 0;
        HIP_CHECK(hipGetDevice(&dev));
        HIP_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        return v;
    }();
    return n;
}

// Would conv2d_stream_forward have put this layer on conv_stream_ws_kernel<1, Cin / 4, NT, 4> (conv_stream.hip: its choice of the
// cout tiling, launch_stream_ws's conditions)?  That kernel starts its accumulators at the bias, every other kernel these layers ran
// on adds it last; the answer only picks between the two, so that a layer's result keeps the bits it had.
bool stream_ws_order(const TView& in, const TView& out, const ConvEpilogue& ep) {
    if (in.C < 24 || (in.C & 7) || (long)in.H * in.W < 256) return false;      // one chunk of E = Cin / 4 in {6, 8, 10, 12}
    const long ntiles = (long)cdiv(in.W, 16) * cdiv(in.H, 16) * in.N;
    if (ntiles >= (1l << 20)) return false;
    int NT = 0;
    long best = -1;
    for (int nt = 1; nt <= 4; ++nt) {
        if ((out.C % nt) && out.C < 16) continue;
        const long padded = (long)cdiv(out.C, 16 * nt) * 16 * nt;
        if (best < 0 || padded < best || (padded == best && nt > NT)) { best = padded; NT = nt; }
    }
    if (out.C < NT) return false;
    while (NT > 1 && ntiles * cdiv(out.C, 16 * NT) < 512) --NT;
    if (NT > 3) return false;
    if ((ep.add.p && ep.add.ld != out.ld) || (ep.mask.p && ep.mask.ld != out.ld)) return false;
    if ((size_t)18 * out.W * out.ld * 4 >= (1ull << 31) || (size_t)18 * in.W * in.ld * 4 >= (1ull << 31)) return false;
    return (double)cdiv((int)ntiles, 8) * cdiv(out.C, 16 * NT) >= (double)std::max(pw_cu_count() / 8, 1);
}

// a view whose pixels are one flat array at pitch ld, readable / writable as float4 channel quads
bool flat(const TView& v) {
    return v.p && v.vec && v.d2s <= 1 && !v.sc && v.ld >= v.C && v.nstride == (size_t)v.H * v.W * v.ld;
}

template <int KT, int NT, int EPI>
void launch_form(hipStream_t s, const PointwiseParams& p) {
    constexpr int PXW = 16 * (KT <= 4 ? 4 : 2);
    constexpr auto kern = conv_pointwise_kernel<KT, NT, EPI>;
    const long long nblk = (p.npx + PXW - 1) / PXW;
    int blocks = (int)std::min<long long>((nblk + 3) / 4, resident_blocks<kern>(256));
    // (tests: at most that many workgroups, so that small grids walk several blocks per wave; it only lowers the grid)
    if (const char* g = test_env("DL4DS_POINTWISE_GRID")) blocks = std::max(1, std::min(blocks, atoi(g)));
    DL4DS_LAUNCH(kern, dim3(blocks), dim3(256), 0, s, p);
    HIP_CHECK(hipGetLastError());
}

template <int KT, int NT>
void launch_pointwise(hipStream_t s, const PointwiseParams& p, int epi) {
#define POINTWISE_FORM(E_) case E_: launch_form<KT, NT, E_>(s, p); break;
    switch (epi) {      // (the forms conv2d_pointwise_form_ok lets through)
        POINTWISE_FORM(0) POINTWISE_FORM(PW_RELU) POINTWISE_FORM(PW_ADD) POINTWISE_FORM(PW_ADD | PW_RELU)
        POINTWISE_FORM(PW_MASK) POINTWISE_FORM(PW_ACC) POINTWISE_FORM(PW_MASK | PW_ACC)
        default: throw Dl4dsError("conv_pointwise: epilogue form " + std::to_string(epi) + " is not built");
    }
#undef POINTWISE_FORM
}

template <int KT>
void dispatch_nt(hipStream_t s, const PointwiseParams& p, int epi) {
    switch ((p.Cout + 15) / 16) {
        case 1: launch_pointwise<KT, 1>(s, p, epi); break;
        case 2: launch_pointwise<KT, 2>(s, p, epi); break;
        default: launch_pointwise<KT, 3>(s, p, epi); break;
    }
}

}  // namespace

// launch half of the pointwise path: conv2d_forward_route (conv_route.h) says which calls come here
void conv2d_pointwise_forward(hipStream_t s, const TView& in, const float* w, const TView& out, const ConvEpilogue& ep) {
    DL4DS_REQUIRE(conv_route::pointwise_ok(in, out, 1, ep), "conv_pointwise: not a call of this family (conv2d_forward_route)");
    DL4DS_REQUIRE(flat(in) && flat(out) && (!ep.add.p || flat(ep.add)) && (!ep.mask.p || flat(ep.mask)), "conv_pointwise: views");
    PointwiseParams p;
    p.x = in.p; p.y = out.p; p.add = ep.add.p; p.mask = ep.mask.p; p.w = w; p.bias = ep.bias;
    p.npx = (long long)in.N * in.H * in.W;
    p.Cin = in.C; p.Cout = out.C;
    p.ldx = in.ld; p.ldy = out.ld; p.lda = ep.add.p ? ep.add.ld : 0; p.ldm = ep.mask.p ? ep.mask.ld : 0;
    p.bias_first = stream_ws_order(in, out, ep) ? 1 : 0;
    const int epi = (ep.add.p ? PW_ADD : 0) | (ep.relu ? PW_RELU : 0) | (ep.mask.p ? PW_MASK : 0) | (ep.accumulate ? PW_ACC : 0);
    const int KT = in.C / 4, NT = (out.C + 15) / 16;
    const double px = (double)p.npx;
    ProfScope ps(s, "conv_pointwise<" + std::to_string(KT) + "," + std::to_string(NT) + ">", 2.0 * px * in.C * out.C,
                 4.0 * (px * (in.C + out.C * (1 + (ep.add.p ? 1 : 0) + (ep.mask.p ? 1 : 0) + (ep.accumulate ? 1 : 0))) +
                        (double)in.C * out.C));
    switch (KT) {
        case 1: dispatch_nt<1>(s, p, epi); break;
        case 2: dispatch_nt<2>(s, p, epi); break;
        case 3: dispatch_nt<3>(s, p, epi); break;
        case 4: dispatch_nt<4>(s, p, epi); break;
        case 5: dispatch_nt<5>(s, p, epi); break;
        case 6: dispatch_nt<6>(s, p, epi); break;
        case 7: dispatch_nt<7>(s, p, epi); break;
        case 8: dispatch_nt<8>(s, p, epi); break;
        case 9: dispatch_nt<9>(s, p, epi); break;
        case 10: dispatch_nt<10>(s, p, epi); break;
        case 11: dispatch_nt<11>(s, p, epi); break;
        default: dispatch_nt<12>(s, p, epi); break;
    }
}
