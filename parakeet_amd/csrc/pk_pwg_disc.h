// pk_pwg_disc.h -- geometry of the fused Parallel WaveGAN discriminator kernel (pwg_disc.hip).
//
// One workgroup of 256 threads carries a window of PWGD_W(C) samples of one utterance through every layer in LDS; the
// window is an output tile plus the receptive field (halo) on both sides, tile = window - 2 * halo.  Two activation
// buffers of (conv_channels rounded up to 32) x window floats have to fit the 160 KiB of a CU, hence the two window sizes.
#pragma once

constexpr int PWGD_THREADS = 256;
constexpr int PWGD_MIN_TILE = 32;        // the smallest output tile a window may be left with
constexpr int PWGD_MAX_LAYERS = 16;
constexpr int PWGD_MAX_K = 9;
// window (samples) of a model with C channels
constexpr int pwgd_window(int C) { return C <= 64 ? 256 : 128; }
// the largest total halo (k - 1) / 2 * (sum of the hidden dilations + 1) per side: 112 samples up to 64 channels, 48 above
constexpr int pwgd_max_halo(int C) { return (pwgd_window(C) - PWGD_MIN_TILE) / 2; }
