// Nearest 2x up-sampling + channel concatenation in one launch, and its backward (gfx950).
// Called by rfn_hip.ops (the skip connections of the upscaler).
#include "common.h"
#include "../../include/rfn_hip.h"

// ---------------------------------------------------------------------------- nearest 2x up-sampling + channel cat
// The upscaler's NearestUp2x -> torch.cat((x, skip), 1) in one launch: out[n, c] = up2x(x[n, c]) for c < Cx, else
// skip[n, c - Cx].  Backward: gx = the 2x2 block sums of g[:, :Cx], read in place through g's frame stride (each sum is
// formed in fp64 and rounded once); the skip's gradient is the view g[:, Cx:].  VEC == 4: 16-byte pieces of the 2w-wide
// rows (w even, aligned pointers and frame strides); VEC == 1: one element per thread.
constexpr int UP2X_GRID_CAP = 8192;
template <int VEC>
__global__ void up2x_cat_kernel(const float* __restrict__ x, long x_ns, const float* __restrict__ skip, long s_ns,
                                float* __restrict__ out, unsigned nunits, int Cx, int Cs, int h, int w) {
    const unsigned upr = VEC == 4 ? (unsigned)w / 2 : 2u * w, H2 = 2u * h, Ct = (unsigned)(Cx + Cs);
    for (unsigned u = blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += gridDim.x * blockDim.x) {
        const unsigned row = u / upr, k = u - row * upr;  // row = (n * Ct + c) * 2h + Y
        const unsigned rc = row / H2, Y = row - rc * H2;
        const unsigned n = rc / Ct, c = rc - n * Ct;
        if (VEC == 4) {
            float4 v;
            if (c < (unsigned)Cx) {
                const float2 t = *reinterpret_cast<const float2*>(x + n * x_ns + ((long)c * h + Y / 2) * w + 2 * k);
                v = float4{t.x, t.x, t.y, t.y};
            } else {
                v = *reinterpret_cast<const float4*>(skip + n * s_ns + ((long)(c - Cx) * H2 + Y) * (2 * w) + 4 * k);
            }
            *reinterpret_cast<float4*>(out + 4ul * u) = v;
        } else {
            out[u] = c < (unsigned)Cx ? x[n * x_ns + ((long)c * h + Y / 2) * w + k / 2]
                                      : skip[n * s_ns + ((long)(c - Cx) * H2 + Y) * (2 * w) + k];
        }
    }
}
template <int VEC>
__global__ void up2x_cat_bwd_kernel(const float* __restrict__ g, long g_ns, float* __restrict__ gx, unsigned nunits,
                                    int Cx, int h, int w) {
    const unsigned upr = VEC == 4 ? (unsigned)w / 2 : (unsigned)w;
    for (unsigned u = blockIdx.x * blockDim.x + threadIdx.x; u < nunits; u += gridDim.x * blockDim.x) {
        const unsigned row = u / upr, k = u - row * upr;  // row = (n * Cx + c) * h + i
        const unsigned rc = row / (unsigned)h, i = row - rc * (unsigned)h;
        const unsigned n = rc / (unsigned)Cx, c = rc - n * (unsigned)Cx;
        const float* r0 = g + n * g_ns + ((long)c * 2 * h + 2 * i) * (2 * w) + (VEC == 4 ? 4 : 2) * k;
        const float* r1 = r0 + 2 * w;
        if (VEC == 4) {
            const float4 a = *reinterpret_cast<const float4*>(r0), b = *reinterpret_cast<const float4*>(r1);
            *reinterpret_cast<float2*>(gx + 2ul * u) = float2{(float)(((double)a.x + a.y) + ((double)b.x + b.y)),
                                                              (float)(((double)a.z + a.w) + ((double)b.z + b.w))};
        } else {
            gx[u] = (float)(((double)r0[0] + r0[1]) + ((double)r1[0] + r1[1]));
        }
    }
}
struct Up2xRoute {
    bool v4;
    long nunits;
    int grid, sweeps;
};
// `aligned`: every pointer is 16-byte aligned and every frame stride a multiple of 4 floats; out_elems = the elements of
// out (forward) or of gx (backward)
static Up2xRoute choose_up2x(long out_elems, int w, int aligned, int bwd) {
    Up2xRoute r;
    r.v4 = w % 2 == 0 && aligned;
    r.nunits = r.v4 ? out_elems / (bwd ? 2 : 4) : out_elems;
    const long nb = (r.nunits + 255) / 256;
    r.grid = (int)(nb < UP2X_GRID_CAP ? nb : UP2X_GRID_CAP);
    r.sweeps = (int)((nb + r.grid - 1) / r.grid);
    return r;
}
static bool up2x_sizes_ok(int N, int Cx, int Cs, int h, int w, int bwd) {
    return N > 0 && Cx > 0 && Cs >= 0 && h > 0 && w > 0 && 4L * N * (bwd ? Cx : Cx + Cs) * h * w < (1L << 31);
}
extern "C" const char* rfn_up2x_cat_kernel_label(int N, int Cx, int Cs, int h, int w, int aligned, int bwd) {
    static thread_local char buf[128];
    if (!up2x_sizes_ok(N, Cx, Cs, h, w, bwd)) return "unsupported";
    const Up2xRoute r = choose_up2x(bwd ? (long)N * Cx * h * w : 4L * N * (Cx + Cs) * h * w, w, aligned, bwd);
    snprintf(buf, sizeof(buf), "up2x_cat%s access=%s grid=%d sweeps=%d", bwd ? "_bwd" : "", r.v4 ? "vec4" : "vec1", r.grid,
             r.sweeps);
    return buf;
}
extern "C" int rfn_up2x_cat_f32(const float* x, long x_ns, const float* skip, long skip_ns, float* out, int N, int Cx,
                                int Cs, int h, int w, rfn_stream_t stream) {
    RFN_CHECK_ARG(x && skip && out && Cs > 0 && up2x_sizes_ok(N, Cx, Cs, h, w, 0), -1);
    RFN_CHECK_ARG(x_ns >= (long)Cx * h * w && skip_ns >= 4L * Cs * h * w, -2);
    const int aligned = ((((uintptr_t)x | (uintptr_t)skip | (uintptr_t)out) & 15) == 0 && x_ns % 4 == 0 && skip_ns % 4 == 0);
    const Up2xRoute r = choose_up2x(4L * N * (Cx + Cs) * h * w, w, aligned, 0);
    launch_vec(r.v4, up2x_cat_kernel<4>, up2x_cat_kernel<1>, dim3(r.grid), (hipStream_t)stream, x, x_ns, skip, skip_ns, out,
               (unsigned)r.nunits, Cx, Cs, h, w);
    RFN_LAUNCH_CHECK();
    return 0;
}
extern "C" int rfn_up2x_cat_bwd_f32(const float* g, long g_ns, float* gx, int N, int Cx, int h, int w,
                                    rfn_stream_t stream) {
    RFN_CHECK_ARG(g && gx && up2x_sizes_ok(N, Cx, 0, h, w, 1), -1);
    RFN_CHECK_ARG(g_ns >= 4L * Cx * h * w, -2);
    const int aligned = ((((uintptr_t)g | (uintptr_t)gx) & 15) == 0 && g_ns % 4 == 0);
    const Up2xRoute r = choose_up2x((long)N * Cx * h * w, w, aligned, 1);
    launch_vec(r.v4, up2x_cat_bwd_kernel<4>, up2x_cat_bwd_kernel<1>, dim3(r.grid), (hipStream_t)stream, g, g_ns, gx,
               (unsigned)r.nunits, Cx, h, w);
    RFN_LAUNCH_CHECK();
    return 0;
}
