// weighted_fusion (reference core/fusion.py:32-35) as scalar device code, shared by the join kernels of csrc/nonlocal_channel.hip and the
// fused attention-fusion kernels of csrc/attn_fuse.hip: one statement of the clamp rule and of torch's division backward.
#pragma once
#include "common.hpp"

namespace mmif {

constexpr float JOIN_EPS = 1e-7f;

struct Wf {  // weighted_fusion(t1, t2, a, b): w = a / max(a + b, eps), f = w t1 + (1 - w) t2
    float w, den, f;
    bool pass;   // the clamp passes gradient to a + b (torch: where a + b >= eps)
};

__device__ inline Wf wf_fwd(float t1, float t2, float a, float b) {
    Wf o;
    const float s = a + b;
    o.pass = s >= JOIN_EPS;
    o.den = s < JOIN_EPS ? JOIN_EPS : s;   // (NaN propagates like clamp)
    o.w = a / o.den;
    o.f = o.w * t1 + (1.f - o.w) * t2;
    return o;
}

// gradients of f = wf(t1, t2, a, b) for upstream df: through the weights only (da, db); the caller adds df w and df (1 - w) to t1 and t2
__device__ inline void wf_bwd(const Wf& o, float t1, float t2, float df, float& da, float& db) {
    const float dw = df * t1 - df * t2;          // torch: grad of w from (w * t1) and from ((1 - w) * t2)
    const float dden = o.pass ? -dw * (o.w / o.den) : 0.f;   // torch's div backward: -grad * ((self / other) / other)
    da = dw / o.den + dden;
    db = dden;
}

}  // namespace mmif
