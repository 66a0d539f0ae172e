// pk_mel.h -- what another translation unit may ask of a pk_mel handle (mel.hip): the Griffin-Lim loop of istft.hip runs
// the forward STFT on the handle's own packed basis instead of building a second copy of it.
#pragma once
#include "pk_common.h"

const pk_mel_cfg* pk_mel_config(const pk_mel* h);
pk_ctx* pk_mel_context(const pk_mel* h);
// pk_gemm_pack of the windowed DFT basis [K = n_fft][N = re(k) | im(k)], device memory owned by the handle
const float* pk_mel_dft_packed(const pk_mel* h);
// PK_TRANSFORM_DENSE or PK_TRANSFORM_FFT; under FFT the fp32 window on the device (n_fft floats)
int pk_mel_transform(const pk_mel* h);
const float* pk_mel_window(const pk_mel* h);
