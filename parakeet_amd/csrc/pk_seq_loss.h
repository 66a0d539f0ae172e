// pk_seq_loss.h -- the tiles of the sequence-loss reductions (seq_loss.hip) and what the tests' bounds read from them.
#pragma once

// pk_pair_loss_run / pk_bce_logits_run: entries of one utterance (row-major over its rows x W rectangle) per workgroup.
// 256 lanes x PK_SEQ_LOSS_VEC consecutive entries x PK_SEQ_LOSS_PAIR_ITERS rounds.
#define PK_SEQ_LOSS_VEC 4
#define PK_SEQ_LOSS_PAIR_ITERS 4
#define PK_SEQ_LOSS_PAIR_TILE (256 * PK_SEQ_LOSS_VEC * PK_SEQ_LOSS_PAIR_ITERS)
#define PK_SEQ_LOSS_MAX_W 8192
// pk_guided_attn_run: one workgroup owns PK_SEQ_LOSS_GUIDE_ROWS rows (s) x PK_SEQ_LOSS_GUIDE_COLS columns (t) of all of an
// utterance's maps; a lane holds the guide of PK_SEQ_LOSS_VEC consecutive columns of one row.
#define PK_SEQ_LOSS_GUIDE_ROWS 16
#define PK_SEQ_LOSS_GUIDE_COLS 64
#define PK_SEQ_LOSS_MAX_MAPS 4096
// Length of the longest chain of fp32 additions in any of the three reductions.  0: every term is formed in fp32 (or, for
// the stop-token term, in fp64) and enters a float64 accumulator at once; lanes, waves, tiles are all combined in float64.
#define PK_SEQ_LOSS_F32_CHAIN 0
