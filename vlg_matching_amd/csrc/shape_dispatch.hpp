// Where a kernel instantiation is chosen from the shape of an index: plain or rrr bit-vectors, narrow or wide SA indices, SA-order or
// text-order samples, the width of the ISA samples, member trails on or off.  A launch site names its kernel ONCE, inside a generic
// lambda that receives the chosen types as tags:
//     return on_bv(iv.bv_kind, [&](auto bv) { return launch(wt_rank_kernel<tag_t<decltype(bv)>>, grid, stream, iv, ...); });
// The combinations that are not full products are written out here and nowhere else, so the set of instantiations does not depend on
// how a site nests its calls.
#pragma once
#include <type_traits>
#include "lf_walk.hpp"

namespace vlg {

template <class T> struct type_tag { using type = T; };
template <bool B> using flag_tag = std::integral_constant<bool, B>;       // read as decltype(flag)::value
template <class Tag> using tag_t = typename Tag::type;

template <class F> auto on_bv(uint32_t bv_kind, F&& f) { return bv_kind == kBvRrr63 ? f(type_tag<RrrBV>{}) : f(type_tag<PlainBV>{}); }
template <class F> auto on_flag(bool b, F&& f) { return b ? f(flag_tag<true>{}) : f(flag_tag<false>{}); }

// the LF walk of the locate family on a byte index (Walk): the quad image where the view carries one, the binary tree otherwise.  A
// caller that wants the binary walk on an index with an image passes a view without it (without_quad)
template <bool kWide, class F> auto on_byte_walk(const IndexView& iv, F&& f)
{
    if (iv.qblocks && iv.bv_kind == kBvPlain) return f(type_tag<QuadWalk<kWide>>{});
    return on_bv(iv.bv_kind, [&](auto bv) { return f(type_tag<ByteWalk<tag_t<decltype(bv)>, kWide>>{}); });
}
inline IndexView without_quad(IndexView iv) { iv.qblocks = nullptr; iv.qnodes = nullptr; iv.n_qnodes = 0; return iv; }

// byte text access (kWide, isa_t): ISA samples are 8 bytes wide from n = 2^32 on, and SA indices are wide there too
template <class F> auto on_text_access_shape(bool wide, uint32_t isa_bytes, F&& f)
{
    if (isa_bytes == 8) return f(flag_tag<true>{}, type_tag<uint64_t>{});
    return wide ? f(flag_tag<true>{}, type_tag<uint32_t>{}) : f(flag_tag<false>{}, type_tag<uint32_t>{});
}
// ISA samples of a byte index (pos_t, out_t): the width of its SA samples and the width of the ISA samples written
template <class F> auto on_isa_samples_shape(bool wide, uint32_t isa_bytes, F&& f)
{
    if (isa_bytes == 8) return wide ? f(type_tag<uint64_t>{}, type_tag<uint64_t>{}) : f(type_tag<uint32_t>{}, type_tag<uint64_t>{});
    return wide ? f(type_tag<uint64_t>{}, type_tag<uint32_t>{}) : f(type_tag<uint32_t>{}, type_tag<uint32_t>{});
}
// round 0 of the sorted sweep (kTrails, kAhead): the look-ahead exists with member trails only
template <class F> auto on_trails_ahead(bool trails, bool ahead, F&& f)
{
    if (trails && ahead) return f(flag_tag<true>{}, flag_tag<true>{});
    return trails ? f(flag_tag<true>{}, flag_tag<false>{}) : f(flag_tag<false>{}, flag_tag<false>{});
}

// what the host reads off a view before it dispatches
struct IndexShape { bool rrr, wide, text_order; };
inline IndexShape shape(const IndexView& iv) { return {iv.bv_kind == kBvRrr63, iv.sample_bytes == 8, iv.sampling == kSamplingTextOrder}; }
inline IndexShape shape(const IntView& v) { return {v.bv_kind == kBvRrr63, false, v.sampling == kSamplingTextOrder}; }

// 256 threads, no dynamic LDS.  The arguments are converted to the kernel's parameter types; a kernel's default arguments do not reach
// through its address, so every parameter is passed.
template <class... P, class... A>
vlg_status launch(void (*kernel)(P...), dim3 grid, hipStream_t stream, A&&... args)
{
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, static_cast<P>(args)...);
    VLG_HIP_TRY(hipGetLastError());
    return VLG_OK;
}

}  // namespace vlg
