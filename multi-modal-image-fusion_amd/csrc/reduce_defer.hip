// Deferred weight-gradient reductions: see wgrad_reduce.hpp.  The kernel below takes every queued job's slot from the job's map and its sum
// from partial_sum(), like the separate launches: per output the same loads in the same order, so the results are bit-identical.
#include "wgrad_reduce.hpp"
#include <string.h>

namespace mmif {

constexpr int RD_MAXJOBS = 8;
struct RedTable { RedJob j[RD_MAXJOBS]; int start[RD_MAXJOBS + 1]; int n; };

__global__ __launch_bounds__(1024) void reduce_multi_kernel(RedTable T) {
    __shared__ float red[16][64];
    int k = 0;
    while (k + 1 < T.n && (int)blockIdx.x >= T.start[k + 1]) ++k;
    const RedJob& J = T.j[k];
    const int lb = blockIdx.x - T.start[k];
    const int sub = J.sl == 16 ? 0 : threadIdx.x >> 8;              // four 256-thread virtual blocks per launch block when sl == 4
    const int vb = J.sl == 16 ? lb : 4 * lb + sub, vt = J.sl == 16 ? threadIdx.x : (threadIdx.x & 255);
    const int idx = vb < J.nvb ? vb * 64 + (vt & 63) : -1;          // (past the job's last virtual block: no output)
    RedSlot s = {-1, 0, nullptr};
    if (idx >= 0) {
        switch (J.kind) {
            case RedJob::DMA: s = J.dma.slot(idx); break;
            case RedJob::TAPROW: s = J.taprow.slot(idx); break;
            case RedJob::IMAGE_OUT3: s = J.image_out3.slot(idx); break;
            default: s = J.image_out1.slot(idx); break;
        }
    }
    const float t = partial_sum(J.partial, s.off, s.stride, J.G, J.sl, vt, red + 4 * sub);
    if ((vt >> 6) == 0 && s.off >= 0 && s.dst != nullptr) *s.dst = J.accumulate ? *s.dst + t : t;
}

static struct {
    char* arena = nullptr;
    size_t cap = 0, used = 0;
    RedJob jobs[RD_MAXJOBS];
    int n = 0;
    bool active = false;
    const float* last_slot = nullptr;
} g_rd;

float* defer_ws(float* ws, size_t bytes) {
    g_rd.last_slot = nullptr;
    if (!g_rd.active || g_rd.n >= RD_MAXJOBS) return ws;
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (g_rd.used + need > g_rd.cap) return ws;
    float* slot = reinterpret_cast<float*>(g_rd.arena + g_rd.used);
    g_rd.used += need;
    g_rd.last_slot = slot;
    return slot;
}

bool defer_push(const RedJob& job) {
    if (!g_rd.active || g_rd.last_slot == nullptr || job.partial != g_rd.last_slot || g_rd.n >= RD_MAXJOBS) return false;
    g_rd.jobs[g_rd.n++] = job;
    g_rd.last_slot = nullptr;
    return true;
}

}  // namespace mmif

using namespace mmif;

// arena: device memory the queued partial sums live in until the flush (the sum of the queued layers' weight-gradient workspaces; a layer
// that does not fit runs its reduce at once, as without deferral).  Stream-ordered like everything else: producers, flush and consumers of
// dW / db must be on one stream.
extern "C" int mmif_reduce_defer_begin(void* arena, size_t bytes) {
    MMIF_REQUIRE(arena != nullptr && bytes > 0, "reduce_defer_begin: NULL arena");
    // (jobs still queued belong to a backward pass that was abandoned half way -- an exception in the caller -- and are dropped)
    g_rd.arena = (char*)arena; g_rd.cap = bytes; g_rd.used = 0; g_rd.n = 0; g_rd.active = true; g_rd.last_slot = nullptr;
    return MMIF_OK;
}

// run every queued reduce as one launch; keep_deferring != 0: later producers are queued again (into the slots after the ones in use)
extern "C" int mmif_reduce_defer_flush(int32_t keep_deferring, void* stream) {
    int rc = MMIF_OK;
    if (g_rd.n > 0) {
        RedTable T;
        memset(&T, 0, sizeof(T));
        int nb = 0;
        for (int i = 0; i < g_rd.n; ++i) {
            T.j[i] = g_rd.jobs[i];
            T.start[i] = nb;
            nb += g_rd.jobs[i].sl == 16 ? g_rd.jobs[i].nvb : cdiv(g_rd.jobs[i].nvb, 4);
        }
        T.start[g_rd.n] = nb;
        T.n = g_rd.n;
        hipLaunchKernelGGL(reduce_multi_kernel, dim3(nb), dim3(1024), 0, (hipStream_t)stream, T);
        rc = check_launch("reduce_multi");
        g_rd.n = 0;
    }
    g_rd.last_slot = nullptr;
    if (!keep_deferring) { g_rd.active = false; g_rd.used = 0; }
    return rc;
}

extern "C" int32_t mmif_reduce_defer_pending(void) { return g_rd.n; }
