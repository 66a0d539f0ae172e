// pk_mel_loss.h -- the tile of the masked-L1 + SSIM pass (mel_loss.hip) and the sizes that follow from it.
#pragma once

// Output rows per tile.  The staged tile has PK_MEL_LOSS_ROWS + 2 * (window_size / 2) rows.
#define PK_MEL_LOSS_ROWS 16
// Output columns per tile at most; W is cut into ceil(W / cols) equal column tiles.
#define PK_MEL_LOSS_MAX_COLS 128
#define PK_MEL_LOSS_MAX_W 1024
// Largest window: with 16 halo rows and columns the smallest tile (16 columns) still fits the LDS budget below.
#define PK_MEL_LOSS_MAX_WINDOW 33
// Dynamic LDS one workgroup may ask for without opting in to more; two workgroups of it share a CU's 160 KiB.
#define PK_MEL_LOSS_LDS_BUDGET 65536

// LDS floats of one tile: both images staged with their halo, five horizontally filtered moments per staged row, the window.
static inline long pk_mel_loss_lds_floats(int cols, int halo) {
    const long sr = PK_MEL_LOSS_ROWS + 2 * halo, sc = cols + 2 * halo;
    return 2 * sr * sc + 5 * sr * cols + (2 * halo + 1);
}
