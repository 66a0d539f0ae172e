// pk_hifigan.h -- geometry of the HiFi-GAN generator's convolution kernel (hifigan.hip).
//
// One workgroup of 256 threads computes HFG_TILE positions of one utterance for 32 * CT output channels.  The input window,
// tile + 2 * halo positions, is staged in LDS in slabs of HFG_SLAB input channels, [position][channel] with a padded row;
// a wave owns two 32-position tiles per weight fragment.
#pragma once

constexpr int HFG_THREADS = 256;
constexpr int HFG_TILE = 256;                           // output positions of a workgroup; tiles start at utterance-relative multiples
constexpr int HFG_MAX_HALO = 64;                        // (k - 1) / 2 * dilation at most
constexpr int HFG_WIN = HFG_TILE + 2 * HFG_MAX_HALO;    // the largest window
constexpr int HFG_SLAB = 32;                            // input channels per LDS slab
constexpr int HFG_ROW16 = HFG_SLAB * 2 + 16;            // bytes of a position's row in one fp16 plane (16 bytes of padding)
constexpr int HFG_ROW32 = HFG_SLAB * 4 + 16;            // ... in the fp32 slab
constexpr int HFG_PLANE16 = HFG_WIN * HFG_ROW16;        // bytes of one fp16 plane (hi, then lo)
constexpr int HFG_LDS_F16 = 2 * HFG_PLANE16;            // 61440
constexpr int HFG_LDS_F32 = HFG_WIN * HFG_ROW32;        // 55296
constexpr long HFG_WORKSPACE_CAP = 16L << 30;           // bytes of activations one call may ask for
constexpr float HFG_OUTPUT_SLOPE = 0.01f;               // the LeakyReLU before output_conv is built WITHOUT arguments: its default
                                                        // slope, not negative_slope (as recalled; not checked against a checkpoint)
