// pwg_gen.h -- the shape-generic Parallel WaveGAN path (pwg_gen.hip), called by the pk_pwg_* entry points of pwg.hip
// for every configuration the tuned kernels (in/out 1, kernel 3, residual 64, gate 128, skip 64, aux 80) cannot take,
// and for the default one under the handle option "generic_kernel".
#pragma once
#include "pk_common.h"
#include "pk_synth.h"

struct pwg_gen;   // weights and workspaces of the generic path

// the envelope of the generic path; PK_OK or PK_EUNSUPPORTED with a message that names the limit
int pwg_gen_check(const pk_pwg_cfg& c);
// the shared state of the handle the generic path reads (pk_pwg owns it)
struct pwg_gen_call {
    pk_ctx* ctx;
    const pk_pwg_cfg* cfg;
    int hop;
    int math;                          // PK_PWG_MATH_*
    bool use_norm;
    const float* mu;                   // device, aux_channels
    const float* sigma;
    unsigned long long seed;
    unsigned long long* rng_offset;    // advanced when the noise is drawn internally
    long chunk_samples;
};
int pwg_gen_finalize(pwg_gen** g, pk_ctx* ctx, const pk_pwg_cfg& c, const pk_param_map& params, int hop);
int pwg_gen_infer(pwg_gen* g, const pwg_gen_call& k, const float* mel, const int32_t* frames, int32_t B,
                  const float* noise, float* wav, int32_t flags);
int pwg_gen_debug_read(pwg_gen* g, pk_ctx* ctx, int32_t what, int32_t b, float* host_out, int64_t n_floats);
void pwg_gen_destroy(pwg_gen* g);
