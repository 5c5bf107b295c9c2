// Which kernel family takes a convolution layer: the ONE statement of the dispatch order and of what each family asks of its views.
// conv2d_forward / conv2d_wgrad (conv.hip) launch what the routes say, conv2d_wgrad_workspace_bytes sizes for it, and the graph
// (ChAttOp::on_prepare) plans its fusions by putting the views it will pass to the same functions.  Pure host code: no stream, no
// device query, no static state.  The tile sizes are the kernels' own (a family's tile count has to stay inside fast_div's range).
#pragma once
#include "ops.h"
#include <algorithm>
namespace conv_route {
constexpr int DTX = 32, DTY = 8;        // conv_direct.hip: output tile (one pixel per thread, 256 threads)
constexpr int NTW = 16, NTH = 32;       // conv_narrow.hip: tile width / height
inline int pad_pow2(int c) { int p = 1; while (p < c) p <<= 1; return p; }
// stencil (VALU) kernels, conv_direct.hip: 3x3 layers with a handful of channels
inline bool eligible(const TView& in, const TView& out, int KS) {
    if (KS != 3 || in.d2s > 1 || out.d2s > 1 || in.C < 1 || out.C < 1) return false;
    if ((long)cdiv(in.W, DTX) * cdiv(in.H, DTY) * in.N >= (1l << 20)) return false;      // fast_div range
    return pad_pow2(in.C) * pad_pow2(out.C) <= 8;
}
// a view with a channel affine is only read by the float4 staging path (Cin % 4 == 0, 16-byte aligned)
inline bool affine_ok(const TView& v) { return !v.sc || (v.vec && (v.C & 3) == 0 && v.C >= 4); }
// conv_narrow.hip, <= 8 x <= 8 channels with float4-able outputs: two pixels per MFMA column (1.5x fewer MFMAs, all lanes store);
// the only variant that also takes inputs whose channel count is not a multiple of 4.  Also the only narrow variant that
// reads a view with a channel affine (float4-loadable inputs only) and emits the pooling partial sums.
inline bool narrow_pair_ok(const TView& in, const TView& out, int KS, const ConvEpilogue& ep) {
    if (KS != 3 || in.d2s > 1 || exp_env("DL4DS_NO_PAIR") || exp_env("DL4DS_NO_NARROW")) return false;
    if ((long)cdiv(in.W, NTW) * cdiv(in.H, NTH) * in.N >= (1l << 20)) return false;    // fast_div range
    return in.C <= 8 && out.C <= 8 && (out.C & 3) == 0 && out.vec && (!ep.add.p || ep.add.vec) &&
           (!ep.mask.p || ep.mask.vec) && ((((uintptr_t)ep.bias) & 15) == 0) && (!in.sc || (in.vec && (in.C & 3) == 0));
}
inline bool narrow_wgrad_eligible(const TView& x, const TView& dz, int KS) {
    if (x.sc) return false;                                   // only the dz operand takes a channel affine here
    if (KS != 3 || x.C > 8 || dz.C > 16 || x.d2s > 1 || dz.d2s > 1 || !dz.vec) return false;    // x may be unaligned / Cin % 4 != 0
    return (long)cdiv(x.W, NTW) * cdiv(x.H, NTH) * x.N < (1l << 20);                   // fast_div range
}
// conv_pointwise.hip: 1x1 layers as a stream over the flattened pixels.  Channel counts that are multiples of four, up to 48; every
// operand a float4-able view whose pixels form one flat array (any pitch ld >= C: a channel slice of a wider buffer; no
// depth_to_space, no frame pick, no channel affine); the epilogue one of the built forms -- bias with {nothing, ReLU, residual,
// residual + ReLU, ReLU mask, accumulate, mask + accumulate}.  Everything else keeps the kernels behind the route
// (conv_point_kernel: channel counts that are not multiples of four).  DL4DS_NO_POINTWISE=1 (a test hook: the A/B comparison of
// tests/test_gpu_conv_pointwise.py; any value in an experiments build) switches the family off, and DL4DS_STREAM_FORCE_WS, which
// forces conv_stream_ws_kernel onto small grids, forces it past this family too.
inline bool pointwise_view_ok(const TView& v) {
    return v.p && v.vec && v.d2s <= 1 && !v.sc && v.ld >= v.C && v.nstride == (size_t)v.H * v.W * v.ld;
}
inline bool pointwise_ok(const TView& in, const TView& out, int KS, const ConvEpilogue& ep) {
    if (KS != 1 || test_env("DL4DS_NO_POINTWISE") || test_env("DL4DS_STREAM_FORCE_WS")) return false;
    if ((in.C & 3) || (out.C & 3) || in.C < 4 || out.C < 4 || in.C > 48 || out.C > 48) return false;
    if (!pointwise_view_ok(in) || !pointwise_view_ok(out) || ep.pool || ((((uintptr_t)ep.bias) & 15) != 0)) return false;
    if (ep.add.p && (!pointwise_view_ok(ep.add) || ep.add.C != out.C)) return false;
    if (ep.mask.p && (!pointwise_view_ok(ep.mask) || ep.mask.C != out.C)) return false;
    const int form = (ep.add.p ? 1 : 0) | (ep.relu ? 2 : 0) | (ep.mask.p ? 4 : 0) | (ep.accumulate ? 8 : 0);
    return form == 0 || form == 1 || form == 2 || form == 3 || form == 4 || form == 8 || form == 12;
}
// channels [c0, c1) of the same pixels: a plain view at the tensor's pitch
inline TView channel_slice(const TView& x, int c0, int c1) {
    TView v = x;
    v.p = x.p + c0; v.C = c1 - c0; v.cp = v.C;
    v.vec = ((v.C & 3) == 0) && ((x.ld & 3) == 0) && ((((uintptr_t)v.p) & 15) == 0);
    return v;
}
}  // namespace conv_route

// ---- forward / dgrad.  Direct: conv_direct.hip; NarrowPair: the pair kernel; Narrow: the other kernels of conv_narrow.hip; Pointwise:
// conv_pointwise.hip (1x1); Rest: conv2d_forward's chain split -> wino -> gemm -> stream -> point -> gemm -> general, whose choices read the device and per-stream state.
enum class ConvFwdFamily { Direct, NarrowPair, Narrow, Pointwise, Rest };
struct ConvFwdRoute { ConvFwdFamily family; const char* refusal; };      // refusal: null, or what conv2d_forward throws for the call

inline ConvFwdRoute conv2d_forward_route(const TView& in, const TView& out, int KS, const ConvEpilogue& ep) {
    using namespace conv_route;
    // a handful of channels: HBM-bound stencil
    if (eligible(in, out, KS)) {
        if (!affine_ok(in) || ep.pool) return {ConvFwdFamily::Direct, "conv_direct: channel-affine input needs float4-loadable channels; no pooling partials"};
        // (a residual or mask operand in depth_to_space layout: the stencil kernels step aside)
        if (!(ep.add.p && ep.add.d2s > 1) && !(ep.mask.p && ep.mask.d2s > 1)) return {ConvFwdFamily::Direct, nullptr};
    }
    // 1x1 with float4-able channel counts up to 48 on flat views: HBM stream over the flattened pixels
    if (pointwise_ok(in, out, KS, ep)) return {ConvFwdFamily::Pointwise, nullptr};
    if (!exp_env("DL4DS_NO_NARROW") && KS == 3 && in.C <= 16 && out.C <= 16 && in.d2s <= 1) {
        const bool pair = narrow_pair_ok(in, out, KS, ep);
        // 9..16 input channels that are not a multiple of four (the 13-channel ConvBlock behind TransitionLast 26 -> 13): the halo
        // staging's float4 loads only need dword alignment; channels beyond Cin are masked when the tile is written to LDS
        const bool unaligned_ok = in.C > 8 && !in.sc && !ep.pool && !exp_env("DL4DS_NO_NARROW_UNALIGNED");
        if ((in.vec || pair || unaligned_ok) && (long)cdiv(in.W, NTW) * cdiv(in.H, NTH) * in.N < (1l << 20)) {      // fast_div range
            if (pair) return {ConvFwdFamily::NarrowPair, nullptr};
            return {ConvFwdFamily::Narrow, (in.sc || ep.pool) ? "conv_narrow: channel-affine input / pooling partials need the pair kernel" : nullptr};
        }
    }
    return {ConvFwdFamily::Rest, (in.sc || ep.pool) ? "conv2d: channel-affine input / pooling partials are only implemented by the direct "
                                                       "and narrow-pair kernels (conv2d_forward_route says which layers they take)" : nullptr};
}

// ---- weight gradient, behind the Winograd try (its choice reads per-stream state).  Direct: conv_direct.hip; Narrow:
// conv_narrow_wgrad_kernel, Cin <= 8; NarrowSlices: 9 .. 16 input channels with <= 8 outputs (13 -> 8: ConvBlock_att's first layer in
// the recurrent nets; 16 -> 8 U-Net decoder layers) -- the general kernel runs these with the eight output channels on half of the MFMA's
// rows (nine MFMAs per pixel quad); conv_narrow_wgrad_kernel<8> on the channel slices [0, 8) and [8, C) takes 2 x 3 (rows 8-15 carry
// the pixel below); General: conv.hip's kernels.
enum class WgradFamily { Direct, Narrow, NarrowSlices, General };
struct WgradRoute { WgradFamily family; int slabs; const char* refusal; };      // slabs written at most (per slice; General: plan_wgrad's)

inline WgradRoute conv2d_wgrad_route(const TView& x, const TView& dz, int KS) {
    using namespace conv_route;
    auto slabs = [&](int tw, int th) { return std::max(1, std::min(cdiv(x.W, tw) * cdiv(x.H, th) * x.N, 1024)); };
    if (eligible(x, dz, KS))
        return {WgradFamily::Direct, slabs(DTX, DTY), (affine_ok(x) && !dz.sc) ? nullptr : "conv_direct wgrad: only a float4-loadable x operand may carry a channel affine"};
    if (!exp_env("DL4DS_NO_NARROW")) {
        if (narrow_wgrad_eligible(x, dz, KS)) return {WgradFamily::Narrow, slabs(NTW, NTH), nullptr};
        if (!exp_env("DL4DS_NO_WGRAD_SPLIT") && x.C > 8 && x.C <= 16 && dz.C <= 8 && narrow_wgrad_eligible(channel_slice(x, 0, 8), dz, KS))
            return {WgradFamily::NarrowSlices, slabs(NTW, NTH), nullptr};
    }
    return {WgradFamily::General, 0, (x.sc || dz.sc) ? "wgrad: channel-affine operands are only implemented by the direct (x) and narrow (dz) kernels" : nullptr};
}
