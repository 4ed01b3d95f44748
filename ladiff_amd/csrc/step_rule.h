// The end of a denoiser step, once: guidance, the step's noise and the scheduler update of four columns of one latent row, as specified
// at ladiff_cfg_scheduler_step / _multistep in include/ladiff_hip.h.  cfg_step_kernel (rowops.hip) and TailRole (systolic.hip) call all of
// it, step_tail_kernel (rowops.hip) the loader and the noise.  Which products fuse is still decided per inlining context.
#pragma once
#include "common.h"
#include "noise_gen.h"

namespace ladiff {
enum CoefCol { COEF_ALPHA_S, COEF_SIGMA_S, COEF_K_X0, COEF_K_X, COEF_K_EPS, COEF_K_NOISE, COEF_K_M };    // columns of a coefficient row
static_assert(LADIFF_COEF_STRIDE == 8, "the coefficient row of include/ladiff_hip.h");
struct StepCoef { float sa, sb, kx0, kx, ke, kn, km; };      // the columns in that order, under the names the formulas use
// row `step` of the table; k_m is read only in the multistep form (column 6 means nothing to the one-step rule) and is 0 otherwise
__device__ __forceinline__ StepCoef step_coef(const float* coef, int step, bool multistep) {
    const float* c = coef + (size_t)step * LADIFF_COEF_STRIDE;
    return StepCoef{c[COEF_ALPHA_S], c[COEF_SIGMA_S], c[COEF_K_X0], c[COEF_K_X], c[COEF_K_EPS], c[COEF_K_NOISE], multistep ? c[COEF_K_M] : 0.f};
}

__device__ __forceinline__ f32x4 guide4(const f32x4 eu, const f32x4 ec, float g) {      // eps_u + g (eps_c - eps_u), ladiff.py:487-490
    f32x4 e;
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = eu[k] + g * (ec[k] - eu[k]);
    return e;
}

// z of columns 4 chunk .. of latent t of the launch's prompt b at schedule position `step`: the generator's normals (noise_gen.h), or the
// caller's tensor at float offset `off`, or zeros.  All branches are uniform over a step.
__device__ __forceinline__ f32x4 step_noise4(const NoiseGen& gen, const float* noise, float k_noise, int step, int b, int t, int chunk, size_t off) {
    if (gen.on && k_noise != 0.f) {
        float zz[4]; unsigned prompt;
        const NoiseGen pg = noise_of_prompt(gen, b, prompt);
        noise_normal4(pg, step, prompt, t, chunk, zz);
        return f32x4{zz[0], zz[1], zz[2], zz[3]};
    }
    if (noise != nullptr && k_noise != 0.f) return ld4(noise + off);
    return f32x4{0.f, 0.f, 0.f, 0.f};
}

// A loop from a source motion (ladiff_diffusion_reverse_from): prompt b enters the schedule at position `start`.  Returns whether the
// prompt's rows take the step at `step` at all - false = frozen: the latent row keeps its bits, x0_prev is neither read nor written - and
// makes the step AT `start` first order in the multistep form: k_x0 + k_m stands in for k_x0 (A (1 + 1/(2 r0)) - A/(2 r0) = A) and m1 is
// not read.  Only coefficients change here, never the statements of step_rule4.  DESIGN 8h.
__device__ __forceinline__ bool step_gate(StepCoef& c, int step, int start) {
    if (step == start) { c.kx0 = c.kx0 + c.km; c.km = 0.f; }
    return step >= start;
}

// x <- the step's result, returns this step's data prediction x0.  The one-step rule is ONE statement and `x += k_m m1` one of its own: an
// addend more would re-associate what the compiler contracts.  m1 points to the previous prediction of these columns and is read only
// inside the k_m != 0 branch (the first step finds anything there; in the one-step form the pointer means nothing).  DESIGN 8f, 8g.
__device__ __forceinline__ f32x4 step_rule4(f32x4& x, const f32x4 e, const f32x4 z, const float* m1, const StepCoef& c) {
    f32x4 x0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x0[k] = (x[k] - c.sb * e[k]) / c.sa;
        x[k] = c.kx0 * x0[k] + c.kx * x[k] + c.ke * e[k] + c.kn * z[k];
    }
    if (c.km != 0.f) {
        const f32x4 m = ld4(m1);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] += c.km * m[k];
    }
    return x0;
}
}  // namespace ladiff
