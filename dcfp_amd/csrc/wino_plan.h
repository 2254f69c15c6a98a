// wino_plan.h - the ONE tile plan of the Winograd F(2x2, 3x3) paths (conv_winograd.hip: three passes and the batched
// weight gradient, conv_winograd2.hip: fused forward / dgrad, conv_winograd3.hip: fused weight gradient).  Host code only.
//
// Tiles are numbered (n, tile row, tile column); tile row `trow` owns the output rows ho = trow + d * (trow / d) and
// ho + d (super-blocks of 2d rows, conv_winograd.hip), likewise for columns.  ho is monotone in trow, so along an axis
// of H pixels the tile rows are, in this order,
//   full   both output rows inside the image                                   [0, full)
//   half   only the first one inside: the row components r = 3 (xi = 12..15) of such a tile feed nothing that is stored
//          (A^T = [1 1 1 0; 0 1 -1 -1]: output row 0 is formed from r = 0, 1, 2)  [full, valid)
//   empty  no output inside                                                      [valid, d * ceil(H / 2d))
// The plan enumerates the `valid` prefix only (H = 128, d = 12: 68 of 72 tile rows), with the tile columns rounded up
// to a multiple of 4 (rows of 16-byte quads, tile pairs that never straddle a tile row: the extra tiles have no
// outputs); on a map whose H and W are multiples of 2d it is the full grid.  DCFP_WINO_RAGGED=0 enumerates the full
// grid d * ceil(H / 2d) x d * ceil(W / 2d) everywhere.
#pragma once
#include <stdlib.h>

struct WinoAxis { int full, half, valid, grid; };     // grid = d * ceil(H / 2d)

inline WinoAxis wino_axis(int H, int d) {
    const int k = (H + 2 * d - 1) / (2 * d) - 1;       // the last super-block
    auto clampd = [d](int v) { return v < 0 ? 0 : v > d ? d : v; };
    WinoAxis a;
    a.valid = k * d + clampd(H - 2 * k * d);
    a.full = k * d + clampd(H - (2 * k + 1) * d);
    a.half = a.valid - a.full;
    a.grid = (k + 1) * d;
    return a;
}

// DCFP_WINO_RAGGED: 1 (default) skip the tiles and components a ragged map cannot use, 0 the full grid with all 16
// components (A/B, and the reference the tests compare against).  Latches on first use.
inline bool wino_ragged_on() {
    static const bool v = [] { const char* e = getenv("DCFP_WINO_RAGGED"); return !e || atoi(e) != 0; }();
    return v;
}

// A rectangle of tile positions whose tiles all need the same components: rows3 / cols3 = the row / column components
// r = 3 / s = 3 are needed.  Tile `i` of a region (0 <= i < tiles) is image i / (nr * nc), tile row r0 + (i / nc) % nr,
// tile column c0 + i % nc; the region's tiles occupy the `nblocks` 64-tile blocks from block `tb0` on (the last one
// padded), so that a block never mixes classes.
struct WinoRegion {
    int r0, nr, c0, nc, rows3, cols3;
    long long tiles;
    int tb0, nblocks;
    int components() const { return (rows3 ? 4 : 3) * (cols3 ? 4 : 3); }
};

struct WinoTilePlan {
    int TH, TW;               // enumerated tile rows / columns per image (TW % 4 == 0)
    long long T, T16;         // N * TH * TW, and rounded up to 16 (row length of the transformed tensors)
    WinoAxis rows, cols;
    int nreg;                 // 1: the whole grid with 16 components, numbered (n, trow, tcol) as T counts them
    WinoRegion reg[4];        // the 16-component region first
    long long tblocks;        // 64-tile blocks over all regions
    long long issued;         // components issued over all regions, padding of the blocks not counted
};

// `ragged`: skip empty tiles; `classes`: also cut the grid into component classes (the fused forward / dgrad kernel
// where nothing depends on the plain tile numbering: no transformed input kept on the side)
inline WinoTilePlan wino_tile_plan(int N, int H, int W, int d, bool ragged, bool classes) {
    WinoTilePlan pl;
    pl.rows = wino_axis(H, d);
    pl.cols = wino_axis(W, d);
    pl.TH = ragged ? pl.rows.valid : pl.rows.grid;
    pl.TW = ((ragged ? pl.cols.valid : pl.cols.grid) + 3) / 4 * 4;
    pl.T = (long long)N * pl.TH * pl.TW;
    pl.T16 = (pl.T + 15) / 16 * 16;
    // the full / half column boundary rounded UP to the quads: a half tile in the full class runs all its components
    int fr = pl.TH, fc = pl.TW;
    if (ragged && classes) {
        fr = pl.rows.full;
        fc = (pl.cols.full + 3) / 4 * 4;
        if (fc > pl.TW) fc = pl.TW;
    }
    const int rr[2][2] = {{0, fr}, {fr, pl.TH - fr}}, cc[2][2] = {{0, fc}, {fc, pl.TW - fc}};
    const int order[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};      // (row class, column class): full = 0, half = 1
    pl.nreg = 0;
    pl.tblocks = 0;
    pl.issued = 0;
    for (int i = 0; i < 4; ++i) {
        const int a = order[i][0], b = order[i][1];
        if (rr[a][1] <= 0 || cc[b][1] <= 0) continue;
        WinoRegion& g = pl.reg[pl.nreg++];
        g.r0 = rr[a][0]; g.nr = rr[a][1]; g.c0 = cc[b][0]; g.nc = cc[b][1];
        g.rows3 = a == 0; g.cols3 = b == 0;
        g.tiles = (long long)N * g.nr * g.nc;
        g.tb0 = (int)pl.tblocks;
        g.nblocks = (int)((g.tiles + 63) / 64);
        pl.tblocks += g.nblocks;
        pl.issued += g.tiles * g.components();
    }
    for (int i = pl.nreg; i < 4; ++i) pl.reg[i] = WinoRegion{0, 0, 0, 0, 1, 1, 0, 0x7fffffff, 0};
    return pl;
}
