// Small HBM-bound kernels around the hot path: timestep embedding, fused
// CFG + DDIM update, latent layout conversion, HTSAT input stage (BatchNorm +
// bicubic resize + mel->image fold + 4x4 patch cut), Swin patch-merge gather,
// token mean pool and L2 normalisation.
#include "common.h"
#include <math.h>

namespace c2d {

__global__ void timestep_emb_kernel(const float* t_table, const int* step_index, int n, int dim, f16* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int half = dim / 2;
    if (i >= n * half) return;
    const int j = i % half, row = i / half;
    const float t = t_table[step_index ? *step_index : 0];
    // diffusers get_timestep_embedding: exp(-ln(1e4) * j / half), fp32
    const float f = expf(-9.210340371976184f * (float)j / (float)half);
    const float a = t * f;
    out[(size_t)row * dim + j] = (f16)cosf(a);
    out[(size_t)row * dim + half + j] = (f16)sinf(a);
}

__global__ void cfg_ddim_kernel(const f16* eps, float* x, int b, int c, int hw, float gsc, const float* coef,
                                const int* step_index) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b * c * hw) return;
    const int p = i % hw, ch = (i / hw) % c, bi = i / (hw * c);
    const int st = *step_index;
    const float a_t = coef[st * 2], a_p = coef[st * 2 + 1];
    const float eu = (float)eps[((size_t)bi * hw + p) * c + ch];
    const float ec = (float)eps[((size_t)(b + bi) * hw + p) * c + ch];
    const float e = eu + gsc * (ec - eu);
    const float xv = x[i];
    const float x0 = (xv - sqrtf(1.0f - a_t) * e) / sqrtf(a_t);
    x[i] = sqrtf(a_p) * x0 + sqrtf(1.0f - a_p) * e;
}

__global__ void step_advance_kernel(int* step_index) { *step_index += 1; }

__global__ void latent_to_nhwc_kernel(const float* x, int n, int c, int hw, int cpad, int dup, f16* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * hw * cpad) return;
    const int ch = i % cpad, p = (i / cpad) % hw, bi = i / (cpad * hw);
    const float v = ch < c ? x[((size_t)bi * c + ch) * hw + p] : 0.f;
    out[i] = (f16)v;
    if (dup) out[(size_t)n * hw * cpad + i] = (f16)v;
}

__global__ void add_kernel(const f16x8* a, const f16x8* b, f16x8* o, size_t n8) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i < n8; i += (size_t)gridDim.x * blockDim.x) o[i] = a[i] + b[i];
}

// torch upsample_bicubic2d cubic convolution, A = -0.75
__device__ __forceinline__ float cc1(float x) { const float A = -0.75f; return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cc2(float x) { const float A = -0.75f; return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

__global__ void mel_patches_kernel(const float* mel, int b, int T, const float* bn_scale, const float* bn_shift, f16* out) {
    // out [b*4096][64]: token (py, px), column k = dy*4 + dx (16 used)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b * 4096 * 64) return;
    const int col = i & 63, tok = (i >> 6) & 4095, bi = i >> 18;
    float val = 0.f;
    if (col < 16) {
        const int dy = col >> 2, dx = col & 3;
        const int py = tok >> 6, px = tok & 63;
        const int r = 4 * py + dy, cidx = 4 * px + dx;      // image row / col in 256x256
        const int tt = (r >> 6) * 256 + cidx;                // time index in [0, 1024)
        const int f = r & 63;                                // mel bin
        const float* m = mel + (size_t)bi * T * 64;
        const float sc = bn_scale[f], sh = bn_shift[f];
        if (T == 1024) {
            val = m[(size_t)tt * 64 + f] * sc + sh;
        } else {
            const float scale = (float)(T - 1) / 1023.f;     // align_corners = True
            const float real = scale * (float)tt;
            const int i0 = (int)floorf(real);
            const float u = real - (float)i0;
            const float w0 = cc2(u + 1.f), w1 = cc1(u), w2 = cc1(1.f - u), w3 = cc2(2.f - u);
            float acc = 0.f;
            const float ws[4] = {w0, w1, w2, w3};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int idx = min(max(i0 - 1 + q, 0), T - 1);
                acc += ws[q] * (m[(size_t)idx * 64 + f] * sc + sh);
            }
            val = acc;
        }
    }
    out[i] = (f16)val;
}

__global__ void patch_merge_kernel(const f16* x, int b, int h, int w, int c, f16* out) {
    // one thread per 8-channel chunk of an output token: out [b][h/2*w/2][4c]
    const int nch = c >> 3;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int h2 = h / 2, w2 = w / 2;
    const size_t total = (size_t)b * h2 * w2 * 4 * nch;
    if (i >= total) return;
    const int ch = i % nch;
    const int part = (i / nch) % 4;
    const size_t tok = i / (4 * nch);
    const int bi = tok / (h2 * w2), r = tok % (h2 * w2);
    const int oy = r / w2, ox = r % w2;
    // torch.cat([x[:, row::2, col::2] for col in range(2) for row in range(2)])
    const int col = part >> 1, row = part & 1;
    const int iy = 2 * oy + row, ix = 2 * ox + col;
    const f16x8 v = *reinterpret_cast<const f16x8*>(x + (((size_t)bi * h + iy) * w + ix) * c + ch * 8);
    *reinterpret_cast<f16x8*>(out + tok * 4 * c + part * c + ch * 8) = v;
}

__global__ void row_mean_kernel(const f16* x, int b, int rows, int c, int ld, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b * c) return;
    const int bi = i / c, ch = i % c;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += (float)x[((size_t)bi * rows + r) * ld + ch];
    out[i] = s / (float)rows;
}

__global__ void l2norm_kernel(float* x, int m, int c) {
    const int row = blockIdx.x;
    __shared__ float part[4];
    float s = 0.f;
    for (int j = threadIdx.x; j < c; j += blockDim.x) s += x[(size_t)row * c + j] * x[(size_t)row * c + j];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    float tot = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) tot += part[i];
    const float inv = 1.0f / fmaxf(sqrtf(tot), 1e-12f);
    for (int j = threadIdx.x; j < c; j += blockDim.x) x[(size_t)row * c + j] *= inv;
}

// Row softmax for the materialised single-head attention of the VAE mid block
// (diffusers Attention with one 512-wide head: softmax(Q K^T / sqrt(d)) over 4096 /
// 9216 keys; the 1/sqrt(d) is folded into to_q).  One 256-thread workgroup per row,
// the row held in registers (NCH 16-B chunks per thread): fp32 max, exp2, sum, scale,
// fp16 out -- one HBM read and one write per score.
template <int NCH>
__global__ void __launch_bounds__(256) softmax_rows_kernel(const f16* x, int cols, int ld, f16* out, int ldo) {
    const size_t row = blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ float part[4];
    f16x8 v[NCH];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c0 = (i * 256 + tid) * 8;
        if (c0 < cols) {
            v[i] = *reinterpret_cast<const f16x8*>(x + row * ld + c0);
#pragma unroll
            for (int j = 0; j < 8; ++j) mx = fmaxf(mx, (float)v[i][j]);
        }
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) part[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    __syncthreads();
    const float L2E = 1.4426950408889634f, ml = mx * L2E;
    float e[NCH][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c0 = (i * 256 + tid) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            e[i][j] = c0 < cols ? __builtin_amdgcn_exp2f(fmaf((float)v[i][j], L2E, -ml)) : 0.f;
            sum += e[i][j];
        }
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    const float inv = 1.0f / (part[0] + part[1] + part[2] + part[3]);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c0 = (i * 256 + tid) * 8;
        if (c0 < cols) {
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (f16)(e[i][j] * inv);
            *reinterpret_cast<f16x8*>(out + row * ldo + c0) = o;
        }
    }
}

// Weight prepack: fp32 [cout][cin][k][k] (PyTorch
// conv / linear layout, k = 1 for a linear) -> fp16 [cout][kpad], K ordered
// (ky, kx, channel) over cin_pad channels (channels >= cin and K >= k*k*cin_pad are 0).
__global__ void pack_weights_kernel(const float* __restrict__ w, int cout, int cin, int ksz, int cin_pad, int kpad,
                                    f16* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)cout * kpad) return;
    const int o = (int)(i / kpad), kk = (int)(i - (size_t)o * kpad);
    float v = 0.f;
    if (kk < ksz * ksz * cin_pad) {
        const int tap = kk / cin_pad, c = kk - tap * cin_pad;
        const int ky = tap / ksz, kx = tap - ky * ksz;
        if (c < cin) v = w[(((size_t)o * cin + c) * ksz + ky) * ksz + kx];
    }
    out[i] = (f16)v;
}

// uint8 NHWC [n][hw][3] -> fp16 NHWC [n][hw][8], (u / 127.5 - 1) in channels 0..2, zeros above: one pixel per
// thread, one 16-B store (the VAE encoder's conv_in reads 8-channel pixels)
__global__ void image_to_nhwc_kernel(const uint8_t* __restrict__ img, size_t npix, f16x8* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    f16x8 v;
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = (f16)0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (f16)((float)img[i * 3 + c] / 127.5f - 1.0f);
    out[i] = v;
}

// DiagonalGaussianDistribution.sample (or .mode) * scaling, NHWC fp16 moments -> NCHW fp32 latents, and
// DDIMScheduler.add_noise at the step the device counter names: one thread per (image, channel, pixel)
__global__ void vae_posterior_noise_kernel(const f16* __restrict__ mom, int ld, const float* __restrict__ eps,
                                           const float* __restrict__ noise, const float* __restrict__ coef,
                                           const int* __restrict__ step_index, int n, int hw, float scaling,
                                           float* __restrict__ x) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * 4 * hw) return;
    const int p = (int)(i % hw), ch = (int)((i / hw) & 3);
    const size_t bi = i / ((size_t)4 * hw);
    const f16* row = mom + (bi * hw + p) * ld;
    float z = (float)row[ch];
    if (eps) {
        const float lv = fminf(fmaxf((float)row[4 + ch], -30.0f), 20.0f);
        z += expf(0.5f * lv) * eps[i];
    }
    z *= scaling;
    if (noise) {
        const float a = coef[2 * (*step_index)];
        z = sqrtf(a) * z + sqrtf(1.0f - a) * noise[i];
    }
    x[i] = z;
}

// The inpainting step's last launch: cfg_ddim_kernel's update (the same roundings, so a pixel with mask 1 gets
// that kernel's bits) blended with the original re-noised to the next step's timestep, or the original
// itself at the last step.  One thread per (image, latent pixel): one 8-byte load each of the uncond and cond
// eps pixel, one mask load, four channel updates (each channel's accesses to x / z0 / noise are coalesced).
// x is read and written in place, so it carries no __restrict__.
__global__ void cfg_ddim_masked_kernel(const f16x4* __restrict__ eps, float* x, const float* __restrict__ z0,
                                       const float* __restrict__ noise, const float* __restrict__ mask, int b, int hw,
                                       int steps, float gsc, const float* __restrict__ coef,
                                       const int* __restrict__ step_index) {
    // cfg_ddim_kernel's source expressions leave the compiler free to fuse multiply-adds, and the same source
    // fuses differently inside this kernel.  So contraction is off and the roundings are spelled out as that
    // kernel's ISA performs them: e and x - sqrt(1 - a_t) e each one fused multiply-add, the final sum two
    // rounded products and an add.  The pairing is pinned by tests/test_inpaint_gpu.py (mask 1 must give
    // c2d_cfg_ddim_step's bits): if a compiler upgrade breaks that test, re-derive this sequence from
    // cfg_ddim_kernel's ISA.
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)b * hw) return;
    const int st = *step_index;
    if ((unsigned)st >= (unsigned)steps) return;   // a counter outside the table: nothing is read or written
    const size_t bi = i / hw, p = i - bi * hw;
    const float a_t = coef[st * 2], a_p = coef[st * 2 + 1];
    const bool last = st == steps - 1;
    const f16x4 vu = eps[i], vc = eps[(size_t)b * hw + i];
    const float m = mask[i];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const size_t j = (bi * 4 + ch) * hw + p;
        const float eu = (float)vu[ch];
        const float ec = (float)vc[ch];
        const float e = fmaf(gsc, ec - eu, eu);
        const float x0 = fmaf(-sqrtf(1.0f - a_t), e, x[j]) / sqrtf(a_t);
        const float xn = sqrtf(a_p) * x0 + sqrtf(1.0f - a_p) * e;
        const float z = z0[j];
        const float known = last ? z : sqrtf(a_p) * z + sqrtf(1.0f - a_p) * noise[j];
        x[j] = (1.0f - m) * known + m * xn;
    }
}

// The DPM-Solver++(2M) step's last launch: classifier-free guidance and the multistep update, and with MASKED
// the inpainting blend on top of the identical arithmetic (a pixel with mask 1 gets the unmasked kernel's bits).
// Contraction is off and every rounding is written out, so the two instantiations cannot fuse differently.
// One thread per (image, latent pixel), as cfg_ddim_masked_kernel: one 8-byte load each of the uncond and cond
// eps pixel, four channel updates with coalesced fp32 accesses.  x and x0_prev are read and written in place
// (each thread its own elements), so neither carries __restrict__.  mcoef row (c2d.h): alpha_s, sigma_s, alpha_t,
// sigma_t, sigma_t / sigma_s, alpha_t (1 - exp(-h)), 1 / (2 r), order.
template <bool MASKED>
__global__ void cfg_dpm_kernel(const f16x4* __restrict__ eps, float* x, float* x0_prev,
                               const float* __restrict__ z0, const float* __restrict__ noise,
                               const float* __restrict__ mask, int b, int hw, int steps, float gsc,
                               const float* __restrict__ mcoef, const int* __restrict__ step_index,
                               const int* __restrict__ first_step) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)b * hw) return;
    const int st = *step_index;
    if ((unsigned)st >= (unsigned)steps) return;   // a counter outside the table: nothing is read or written
    const size_t bi = i / hw, p = i - bi * hw;
    const float* row = mcoef + (size_t)st * 8;
    const float alpha_s = row[0], sigma_s = row[1], alpha_t = row[2], sigma_t = row[3];
    const float ratio = row[4], gain = row[5], inv2r = row[6];
    const bool first_order = st == *first_step || row[7] == 1.0f;   // x0_prev is not read then: it may hold anything
    const bool last = st == steps - 1;
    const f16x4 vu = eps[i], vc = eps[(size_t)b * hw + i];
    float m = 1.0f;
    if constexpr (MASKED) m = mask[i];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const size_t j = (bi * 4 + ch) * hw + p;
        const float eu = (float)vu[ch];
        const float ec = (float)vc[ch];
        const float e = eu + gsc * (ec - eu);
        const float xv = x[j];
        const float x0 = (xv - sigma_s * e) / alpha_s;
        float d = x0;
        if (!first_order) d = x0 + (x0 - x0_prev[j]) * inv2r;
        float xn = ratio * xv + gain * d;
        if constexpr (MASKED) {
            const float z = z0[j];
            const float known = last ? z : alpha_t * z + sigma_t * noise[j];
            xn = (1.0f - m) * known + m * xn;
        }
        x0_prev[j] = x0;
        x[j] = xn;
    }
}

// uint8 mask [n][8h][8w] -> fp32 [n][h][w]: the sample at (8y, 8x) (F.interpolate nearest at an exact factor 8),
// binarised at 128
__global__ void mask_to_latent_kernel(const uint8_t* __restrict__ mask, int n, int h, int w, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * h * w) return;
    const size_t xo = i % w, yo = (i / w) % h, bi = i / ((size_t)w * h);
    out[i] = mask[(bi * 8 * h + 8 * yo) * 8 * w + 8 * xo] >= 128 ? 1.0f : 0.0f;
}

// out pixel = mask >= 128 ? decoded : original, uint8 RGB; each thread reads its pixel of both images before it
// writes, so out may be decoded (no __restrict__ on either)
__global__ void composite_u8_kernel(const uint8_t* decoded, const uint8_t* __restrict__ original,
                                    const uint8_t* __restrict__ mask, size_t npix, uint8_t* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const bool repaint = mask[i] >= 128;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = repaint ? decoded[i * 3 + c] : original[i * 3 + c];
}

// The entry into the inpainting loop in one launch: vae_posterior_noise_kernel's z0 (kept, the masked step blends
// with it), the loop's first latents x (z0 noised to the step the device counter names, or the noise itself
// when the loop starts from pure noise) and mask_to_latent_kernel's mask.  One thread per (image, latent pixel):
// its 8 moments are the first 16 bytes of its row; the four channel accesses to eps / noise / z0 / x are each
// coalesced across the wave (consecutive lanes, consecutive pixels of one channel plane), as in
// cfg_ddim_masked_kernel.  The outputs are __restrict__: x must not alias noise or z0 (c2d.h).
__global__ void inpaint_prepare_kernel(const f16* __restrict__ mom, int ld, const float* __restrict__ eps,
                                       const float* __restrict__ noise, const uint8_t* __restrict__ mask_u8,
                                       const float* __restrict__ coef, const int* __restrict__ step_index,
                                       int pure_noise, int n, int h, int w, float scaling, float* __restrict__ z0,
                                       float* __restrict__ x, float* __restrict__ mask) {
    const size_t hw = (size_t)h * w;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * hw) return;
    const size_t bi = i / hw, p = i - bi * hw;
    const size_t yo = p / w, xo = p - yo * w;
    float sa = 0.0f, sn = 1.0f;
    if (!pure_noise) {
        const float a = coef[2 * (*step_index)];
        sa = sqrtf(a);
        sn = sqrtf(1.0f - a);
    }
    const f16* row = mom + i * ld;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const size_t j = (bi * 4 + ch) * hw + p;
        float z = (float)row[ch];
        if (eps) {
            const float lv = fminf(fmaxf((float)row[4 + ch], -30.0f), 20.0f);
            z += expf(0.5f * lv) * eps[j];
        }
        z *= scaling;
        const float nz = noise[j];
        z0[j] = z;
        x[j] = pure_noise ? nz : sa * z + sn * nz;
    }
    mask[i] = mask_u8[(bi * 8 * h + 8 * yo) * 8 * w + 8 * xo] >= 128 ? 1.0f : 0.0f;
}

// ---- CLIP image preprocess: uint8 image -> normalised fp16 patch rows (c2d_clip_preprocess, c2d.h) ----
// PIL's bicubic kernel (ImagingResample, a = -0.5)
__device__ __forceinline__ float pil_cubic(float x) {
    const float A = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * A;
    return 0.0f;
}

// a pass's stored byte: floor(v + 0.5) clamped to [0, 255]
__device__ __forceinline__ float round_u8(float v) { return fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f); }

constexpr int kClipMaxPatch = 32;    // patch side: the per-patch tables and the staged row are static LDS
constexpr int kClipChunkRows = 64;   // source rows per horizontal-pass chunk held in LDS

struct ClipPre {
    int h, w;            // source image
    int top, left;       // the crop window's origin in the resized image
    int size, patch, kpad;
    double sx, sy;       // n_in / n_out per axis
    float mean[3], inv_std[3];
};

// One workgroup per (image, patch).  Both passes touch only what this patch's patch x patch outputs need:
//   tables      per output column / row of the patch: the tap range [lo, hi), the centre (double: tap offsets of
//               large images lose bits in fp32) and 1 / (sum of the tap weights); ranges and centres in double with
//               contraction off, the operations of the float64 statement in c2d.h
//   horizontal  source rows [ylo[0], yhi[patch - 1]) in chunks of kClipChunkRows: each (row, column, channel)
//               reads its taps from the image (bytes, channel-interleaved: the lanes of a wave read neighbouring
//               bytes) and stores the rounded byte in LDS
//   vertical    each output element adds its taps of the chunk to its fp32 accumulator (LDS; an element is always
//               visited by the same thread, so the accumulators need no barrier of their own)
//   store       round, normalise, fp16 into the staged row (zero-filled to kpad), then 16-byte stores
// No load leaves the image: tap ranges are clipped to [0, n_in) and chunk rows to yhi[patch - 1] <= h.
__global__ void __launch_bounds__(256) clip_preprocess_kernel(const uint8_t* __restrict__ img, ClipPre a,
                                                              f16* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_c[2][kClipMaxPatch];
    __shared__ int s_lo[2][kClipMaxPatch], s_hi[2][kClipMaxPatch];
    __shared__ float s_inv[2][kClipMaxPatch];
    __shared__ float s_acc[3 * kClipMaxPatch * kClipMaxPatch];
    __shared__ uint8_t s_t[kClipChunkRows * kClipMaxPatch * 3];
    __shared__ __attribute__((aligned(16))) f16 s_row[(3 * kClipMaxPatch * kClipMaxPatch + 63) / 64 * 64];

    const int P = a.patch, g = a.size / P, tid = threadIdx.x;
    const size_t blk = blockIdx.x;
    const int pidx = (int)(blk % (size_t)(g * g));
    const size_t bi = blk / (size_t)(g * g);
    const int py = pidx / g, px = pidx - py * g;
    const float inv_fx = 1.0f / (float)fmax(a.sx, 1.0), inv_fy = 1.0f / (float)fmax(a.sy, 1.0);

    if (tid < 2 * P) {
        const int axis = tid / P, i = tid - axis * P;   // 0: columns, 1: rows
        const int n_in = axis ? a.h : a.w;
        const int o = (axis ? a.top + py * P : a.left + px * P) + i;
        const double scale = axis ? a.sy : a.sx;
        const double fs = fmax(scale, 1.0), support = 2.0 * fs;
        const double centre = ((double)o + 0.5) * scale;
        const int lo = max((int)(centre - support + 0.5), 0);
        const int hi = min((int)(centre + support + 0.5), n_in);
        const float inv_f = axis ? inv_fy : inv_fx;
        float sum = 0.0f;
        for (int j = lo; j < hi; ++j) sum += pil_cubic((float)((double)j + 0.5 - centre) * inv_f);
        s_c[axis][i] = centre;
        s_lo[axis][i] = lo;
        s_hi[axis][i] = hi;
        s_inv[axis][i] = 1.0f / sum;
    }
    const int n_out = 3 * P * P;
    for (int e = tid; e < n_out; e += 256) s_acc[e] = 0.0f;
    __syncthreads();

    const int y0 = s_lo[1][0], y1 = s_hi[1][P - 1];
    const uint8_t* src = img + bi * (size_t)a.h * a.w * 3;
    for (int r0 = y0; r0 < y1; r0 += kClipChunkRows) {
        const int nr = min(kClipChunkRows, y1 - r0);
        for (int idx = tid; idx < nr * P * 3; idx += 256) {
            const int c = idx % 3, x = (idx / 3) % P, jr = idx / (3 * P);
            const uint8_t* row = src + (size_t)(r0 + jr) * a.w * 3 + c;
            const double cx = s_c[0][x];
            float s = 0.0f;
            for (int i = s_lo[0][x]; i < s_hi[0][x]; ++i)
                s += pil_cubic((float)((double)i + 0.5 - cx) * inv_fx) * (float)row[(size_t)i * 3];
            s_t[idx] = (uint8_t)round_u8(s * s_inv[0][x]);
        }
        __syncthreads();
        for (int e = tid; e < n_out; e += 256) {
            const int c = e % 3, dx = (e / 3) % P, dy = e / (3 * P);
            const int lo = max(s_lo[1][dy], r0), hi = min(s_hi[1][dy], r0 + nr);
            const double cy = s_c[1][dy];
            float s = s_acc[e];
            for (int j = lo; j < hi; ++j)
                s += pil_cubic((float)((double)j + 0.5 - cy) * inv_fy) * (float)s_t[((j - r0) * P + dx) * 3 + c];
            s_acc[e] = s;
        }
        __syncthreads();
    }

    for (int e = tid; e < a.kpad; e += 256) {
        float v = 0.0f;
        if (e < n_out) {
            const int c = e % 3, dy = e / (3 * P);
            v = (round_u8(s_acc[e] * s_inv[1][dy]) / 255.0f - a.mean[c]) * a.inv_std[c];
        }
        s_row[e] = (f16)v;
    }
    __syncthreads();
    f16x8* dst = reinterpret_cast<f16x8*>(out + blk * (size_t)a.kpad);
    for (int q = tid; q < a.kpad / 8; q += 256) dst[q] = reinterpret_cast<const f16x8*>(s_row)[q];
}

// out[i] = a_i . b_i / max(|a_i| |b_i|, 1e-12): one workgroup per row pair, fp32 sums
__global__ void __launch_bounds__(256) cosine_rows_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          int c, float* __restrict__ out) {
    const size_t row = blockIdx.x;
    __shared__ float part[3][4];
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int j = threadIdx.x; j < c; j += blockDim.x) {
        const float x = a[row * c + j], y = b[row * c + j];
        ab += x * y;
        aa += x * x;
        bb += y * y;
    }
    ab = wave_sum(ab);
    aa = wave_sum(aa);
    bb = wave_sum(bb);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = ab;
        part[1][threadIdx.x >> 6] = aa;
        part[2][threadIdx.x >> 6] = bb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float d = part[0][0] + part[0][1] + part[0][2] + part[0][3];
        const float na = sqrtf(part[1][0] + part[1][1] + part[1][2] + part[1][3]);
        const float nb = sqrtf(part[2][0] + part[2][1] + part[2][2] + part[2][3]);
        out[row] = d / fmaxf(na * nb, 1e-12f);
    }
}

}  // namespace c2d

using namespace c2d;

extern "C" const char* c2d_version(void) { return "c2d_hip gfx950 r7"; }

extern "C" int c2d_clip_preprocess(const uint8_t* img, int n, int h, int w, int size, int patch, const float* mean,
                                   const float* std, int kpad, void* out, void* stream) {
    if (!img || !mean || !std || !out) return C2D_E_ARG;
    if (n <= 0 || h <= 0 || w <= 0 || size <= 0 || patch <= 0 || patch > kClipMaxPatch || size % patch) return C2D_E_SHAPE;
    if (kpad != (3 * patch * patch + 63) / 64 * 64) return C2D_E_SHAPE;
    for (int c = 0; c < 3; ++c)
        if (!(std[c] > 0.0f)) return C2D_E_ARG;
    const long long g = size / patch, blocks = (long long)n * g * g;
    // the longer resized side, int(size * long / short), must stay an int
    const long long lng = (long long)size * (h > w ? h : w) / (h > w ? w : h);
    if (blocks > INT32_MAX || lng > INT32_MAX) return C2D_E_SHAPE;
    if (!aligned16(out)) return C2D_E_ALIGN;
    ClipPre a;
    a.h = h; a.w = w; a.size = size; a.patch = patch; a.kpad = kpad;
    const int rh = h <= w ? size : (int)lng, rw = h <= w ? (int)lng : size;   // shorter side -> size
    a.top = (rh - size) / 2;
    a.left = (rw - size) / 2;
    a.sy = (double)h / (double)rh;
    a.sx = (double)w / (double)rw;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean[c];
        a.inv_std[c] = 1.0f / std[c];
    }
    hipLaunchKernelGGL(clip_preprocess_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, img, a,
                       (f16*)out);
    return check_launch();
}

extern "C" int c2d_cosine_rows(const float* a, const float* b, int m, int c, float* out, void* stream) {
    if (!a || !b || !out) return C2D_E_ARG;
    if (m <= 0 || c <= 0) return C2D_E_SHAPE;
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) return C2D_E_ALIGN;
    hipLaunchKernelGGL(cosine_rows_kernel, dim3(m), dim3(256), 0, (hipStream_t)stream, a, b, c, out);
    return check_launch();
}

extern "C" int c2d_timestep_embedding(const float* t_table, const int* step_index, int n, int dim, void* out,
                                      void* stream) {
    if (!t_table || !out) return C2D_E_ARG;
    if (dim & 1 || n <= 0) return C2D_E_SHAPE;
    const int tot = n * dim / 2;
    hipLaunchKernelGGL(timestep_emb_kernel, dim3((tot + 255) / 256), dim3(256), 0, (hipStream_t)stream, t_table,
                       step_index, n, dim, (f16*)out);
    return check_launch();
}

extern "C" int c2d_cfg_ddim_step(const void* eps, float* x, int b, int c, int hw, float guidance, const float* coef,
                                 int* step_index, int advance, void* stream) {
    if (!eps || !x || !coef || !step_index) return C2D_E_ARG;
    if (b <= 0 || c <= 0 || hw <= 0) return C2D_E_SHAPE;
    const int tot = b * c * hw;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cfg_ddim_kernel, dim3((tot + 255) / 256), dim3(256), 0, s, (const f16*)eps, x, b, c, hw,
                       guidance, coef, step_index);
    if (advance) hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, step_index);
    return check_launch();
}

extern "C" int c2d_image_to_nhwc(const uint8_t* img, int n, int hw, void* out, void* stream) {
    if (!img || !out) return C2D_E_ARG;
    if (n <= 0 || hw <= 0) return C2D_E_SHAPE;
    if (!aligned16(out)) return C2D_E_ALIGN;
    const size_t npix = (size_t)n * hw;
    hipLaunchKernelGGL(image_to_nhwc_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       img, npix, (f16x8*)out);
    return check_launch();
}

extern "C" int c2d_vae_posterior_noise(const void* moments, int ld, const float* eps, const float* noise,
                                       const float* coef, const int* step_index, int n, int hw, float scaling,
                                       float* x, void* stream) {
    if (!moments || !x || (noise && (!coef || !step_index))) return C2D_E_ARG;
    if (n <= 0 || hw <= 0 || ld < 8) return C2D_E_SHAPE;
    if (((uintptr_t)moments & 1) || ((uintptr_t)x & 3)) return C2D_E_ALIGN;
    const size_t tot = (size_t)n * 4 * hw;
    hipLaunchKernelGGL(vae_posterior_noise_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (const f16*)moments, ld, eps, noise, coef, step_index, n, hw, scaling, x);
    return check_launch();
}

extern "C" int c2d_cfg_ddim_step_masked(const void* eps, float* x, const float* z0, const float* noise,
                                        const float* mask, int b, int hw, int steps, float guidance,
                                        const float* coef, int* step_index, int advance, void* stream) {
    if (!eps || !x || !z0 || !noise || !mask || !coef || !step_index) return C2D_E_ARG;
    if (b <= 0 || hw <= 0 || steps <= 0) return C2D_E_SHAPE;
    if (((uintptr_t)eps & 7) || (((uintptr_t)x | (uintptr_t)z0 | (uintptr_t)noise | (uintptr_t)mask) & 3))
        return C2D_E_ALIGN;
    const size_t tot = (size_t)b * hw;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cfg_ddim_masked_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s,
                       (const f16x4*)eps, x, z0, noise, mask, b, hw, steps, guidance, coef, step_index);
    if (advance) hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, step_index);
    return check_launch();
}

// The checks c2d_cfg_dpm_step and c2d_cfg_dpm_step_masked share; tot = b * hw on success.
static int cfg_dpm_check(const void* eps, const float* x, const float* x0_prev, int b, int hw, int steps,
                         const float* mcoef, const int* step_index, const int* first_step, size_t* tot) {
    if (!eps || !x || !x0_prev || !mcoef || !step_index || !first_step) return C2D_E_ARG;
    if (b <= 0 || hw <= 0 || steps <= 0) return C2D_E_SHAPE;
    *tot = (size_t)b * hw;
    if (*tot > (size_t)INT32_MAX / 4) return C2D_E_SHAPE;   // b * 4 * hw elements stay below 2^31
    const uintptr_t xa = (uintptr_t)x, pa = (uintptr_t)x0_prev, bytes = (uintptr_t)*tot * 4 * sizeof(float);
    if (xa < pa + bytes && pa < xa + bytes) return C2D_E_ARG;   // both are read and written: they must not overlap
    if (((uintptr_t)eps & 7) || ((xa | pa | (uintptr_t)mcoef | (uintptr_t)step_index | (uintptr_t)first_step) & 3))
        return C2D_E_ALIGN;
    return C2D_OK;
}

extern "C" int c2d_cfg_dpm_step(const void* eps, float* x, float* x0_prev, int b, int hw, int steps, float guidance,
                                const float* mcoef, int* step_index, const int* first_step, int advance,
                                void* stream) {
    size_t tot = 0;
    const int rc = cfg_dpm_check(eps, x, x0_prev, b, hw, steps, mcoef, step_index, first_step, &tot);
    if (rc != C2D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cfg_dpm_kernel<false>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s,
                       (const f16x4*)eps, x, x0_prev, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, b, hw, steps, guidance, mcoef, step_index, first_step);
    if (advance) hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, step_index);
    return check_launch();
}

extern "C" int c2d_cfg_dpm_step_masked(const void* eps, float* x, float* x0_prev, const float* z0,
                                       const float* noise, const float* mask, int b, int hw, int steps,
                                       float guidance, const float* mcoef, int* step_index, const int* first_step,
                                       int advance, void* stream) {
    if (!z0 || !noise || !mask) return C2D_E_ARG;
    size_t tot = 0;
    const int rc = cfg_dpm_check(eps, x, x0_prev, b, hw, steps, mcoef, step_index, first_step, &tot);
    if (rc != C2D_OK) return rc;
    if (((uintptr_t)z0 | (uintptr_t)noise | (uintptr_t)mask) & 3) return C2D_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cfg_dpm_kernel<true>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s,
                       (const f16x4*)eps, x, x0_prev, z0, noise, mask, b, hw, steps, guidance, mcoef, step_index,
                       first_step);
    if (advance) hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, step_index);
    return check_launch();
}

extern "C" int c2d_mask_to_latent(const uint8_t* mask_u8, int n, int h, int w, float* out, void* stream) {
    if (!mask_u8 || !out) return C2D_E_ARG;
    if (n <= 0 || h <= 0 || w <= 0) return C2D_E_SHAPE;
    if ((uintptr_t)out & 3) return C2D_E_ALIGN;
    const size_t tot = (size_t)n * h * w;
    hipLaunchKernelGGL(mask_to_latent_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       mask_u8, n, h, w, out);
    return check_launch();
}

extern "C" int c2d_composite_u8(const uint8_t* decoded, const uint8_t* original, const uint8_t* mask_u8, size_t npix,
                                uint8_t* out, void* stream) {
    if (!decoded || !original || !mask_u8 || !out) return C2D_E_ARG;
    if (npix == 0 || npix > (size_t)INT32_MAX) return C2D_E_SHAPE;   // a negative count cast to size_t lands above
    hipLaunchKernelGGL(composite_u8_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       decoded, original, mask_u8, npix, out);
    return check_launch();
}

extern "C" int c2d_inpaint_prepare(const void* moments, int ld, const float* eps, const float* noise,
                                   const uint8_t* mask_u8, const float* coef, const int* step_index, int pure_noise,
                                   int n, int h, int w, float scaling, float* z0, float* x, float* mask,
                                   void* stream) {
    if (!moments || !noise || !mask_u8 || !z0 || !x || !mask || (!pure_noise && (!coef || !step_index)))
        return C2D_E_ARG;
    if (n <= 0 || h <= 0 || w <= 0 || ld < 8) return C2D_E_SHAPE;
    if (((uintptr_t)moments & 1) || (((uintptr_t)eps | (uintptr_t)noise | (uintptr_t)coef | (uintptr_t)step_index |
                                      (uintptr_t)z0 | (uintptr_t)x | (uintptr_t)mask) & 3))
        return C2D_E_ALIGN;
    const size_t tot = (size_t)n * h * w;
    hipLaunchKernelGGL(inpaint_prepare_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const f16*)moments, ld, eps, noise, mask_u8, coef, step_index, pure_noise ? 1 : 0, n, h, w,
                       scaling, z0, x, mask);
    return check_launch();
}

extern "C" int c2d_latent_to_nhwc(const float* x, int n, int c, int hw, int cpad, int dup, void* out, void* stream) {
    if (!x || !out) return C2D_E_ARG;
    if (cpad < c || n <= 0 || c <= 0 || hw <= 0) return C2D_E_SHAPE;
    const int tot = n * hw * cpad;
    hipLaunchKernelGGL(latent_to_nhwc_kernel, dim3((tot + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, n, c,
                       hw, cpad, dup, (f16*)out);
    return check_launch();
}

__global__ void upsample2x_kernel(const f16x8* __restrict__ x, int h, int w, int c8, f16x8* __restrict__ out,
                                  size_t total) {
    // one thread per output 16-byte chunk; consecutive threads walk channels then columns
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int cc = (int)(i % c8);
        const size_t pix = i / c8;
        const int ox = (int)(pix % (2 * w));
        const size_t r = pix / (2 * w);
        const int oy = (int)(r % (2 * h));
        const size_t n = r / (2 * h);
        out[i] = x[((n * h + (oy >> 1)) * w + (ox >> 1)) * c8 + cc];
    }
}

extern "C" int c2d_upsample_nearest2x(const void* x, int n, int h, int w, int c, void* out, void* stream) {
    if (!x || !out) return C2D_E_ARG;
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 7)) return C2D_E_SHAPE;
    if (!aligned16(x) || !aligned16(out)) return C2D_E_ALIGN;
    const size_t total = (size_t)n * 4 * h * w * (c / 8);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(upsample2x_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const f16x8*)x, h, w, c / 8,
                       (f16x8*)out, total);
    return check_launch();
}

extern "C" int c2d_add(const void* a, const void* b, void* out, size_t n, void* stream) {
    if (!a || !b || !out) return C2D_E_ARG;
    if (n & 7) return C2D_E_SHAPE;
    if (!aligned16(a) || !aligned16(b) || !aligned16(out)) return C2D_E_ALIGN;
    const size_t n8 = n / 8;
    const unsigned blocks = (unsigned)((n8 + 255) / 256 < 4096 ? (n8 + 255) / 256 : 4096);
    if (!n8) return C2D_OK;
    hipLaunchKernelGGL(add_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const f16x8*)a, (const f16x8*)b,
                       (f16x8*)out, n8);
    return check_launch();
}

extern "C" int c2d_htsat_mel_patches(const float* mel, int b, int t, const float* bn_scale, const float* bn_shift,
                                     void* out, void* stream) {
    if (!mel || !bn_scale || !bn_shift || !out) return C2D_E_ARG;
    if (b <= 0 || t < 2 || t > 1024) return C2D_E_SHAPE;
    const int tot = b * 4096 * 64;
    hipLaunchKernelGGL(mel_patches_kernel, dim3((tot + 255) / 256), dim3(256), 0, (hipStream_t)stream, mel, b, t,
                       bn_scale, bn_shift, (f16*)out);
    return check_launch();
}

extern "C" int c2d_patch_merge_gather(const void* x, int b, int h, int w, int c, void* out, void* stream) {
    if (!x || !out) return C2D_E_ARG;
    if (b <= 0 || h <= 0 || w <= 0 || c <= 0 || (h & 1) || (w & 1) || (c & 7)) return C2D_E_SHAPE;
    if (!aligned16(x) || !aligned16(out)) return C2D_E_ALIGN;
    const size_t tot = (size_t)b * (h / 2) * (w / 2) * 4 * (c / 8);
    hipLaunchKernelGGL(patch_merge_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const f16*)x, b, h, w, c, (f16*)out);
    return check_launch();
}

extern "C" int c2d_row_mean(const void* x, int b, int rows, int c, int ld, float* out, void* stream) {
    if (!x || !out) return C2D_E_ARG;
    if (b <= 0 || rows <= 0 || c <= 0 || ld < c) return C2D_E_SHAPE;
    const int tot = b * c;
    hipLaunchKernelGGL(row_mean_kernel, dim3((tot + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const f16*)x, b,
                       rows, c, ld, out);
    return check_launch();
}

extern "C" int c2d_l2_normalize(float* x, int m, int c, void* stream) {
    if (!x) return C2D_E_ARG;
    if (m <= 0 || c <= 0) return C2D_E_SHAPE;
    hipLaunchKernelGGL(l2norm_kernel, dim3(m), dim3(256), 0, (hipStream_t)stream, x, m, c);
    return check_launch();
}

extern "C" int c2d_softmax_rows(const void* x, int rows, int cols, int ld, void* out, int ldo, void* stream) {
    if (!x || !out) return C2D_E_ARG;
    if (rows < 0 || cols <= 0 || cols % 8 || cols > 16384 || ld < cols || ldo < cols) return C2D_E_SHAPE;
    if (((uintptr_t)x | (uintptr_t)out) & 15 || ld % 8 || ldo % 8) return C2D_E_ALIGN;
    if (rows == 0) return 0;
    const int nch = (cols / 8 + 255) / 256;
    const hipStream_t s = (hipStream_t)stream;
#define C2D_SM(N) hipLaunchKernelGGL(softmax_rows_kernel<N>, dim3(rows), dim3(256), 0, s, (const f16*)x, cols, ld, (f16*)out, ldo)
    if (nch <= 1) C2D_SM(1);
    else if (nch <= 2) C2D_SM(2);
    else if (nch <= 4) C2D_SM(4);
    else C2D_SM(8);
#undef C2D_SM
    return check_launch();
}

extern "C" int c2d_pack_weights(const float* w, int cout, int cin, int ksize, int cin_pad, int kpad, void* out,
                                void* stream) {
    if (!w || !out) return C2D_E_ARG;
    if (cout <= 0 || cin <= 0 || (ksize != 1 && ksize != 3) || cin_pad < cin || kpad % 64 ||
        kpad < ksize * ksize * cin_pad)
        return C2D_E_SHAPE;
    const size_t n = (size_t)cout * kpad;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       cout, cin, ksize, cin_pad, kpad, (f16*)out);
    return check_launch();
}
