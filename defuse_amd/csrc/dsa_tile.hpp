// dsa_tile.hpp — the tile width in use of the split-read kernels (pure arithmetic, host and device).
//
// The register tile of the fill has room for TILE_W = 64 reference columns, but a window is rarely a multiple of 64: a
// 389-base window is 6 x 64 + 5, so seven 64-column passes sweep 448 columns for 389 real ones.  An upload is therefore
// swept with a width in use WT <= 64 — columns WT..63 of a tile do not exist — chosen so that the columns swept for its
// widest window, ceil(L / WT) * WT, are fewest (389: seven tiles of 56 = 392).  Every fill launch uses the one
// instantiation of the kernels for its WT.
#pragma once

namespace dsa {

constexpr int TILE_W = 64;                             // storage width of a tile: reference codes, table rows, column masks
// The widths the kernels are instantiated for, widest first.  (52 and 48 are not built: with 60 and 56 they would double
// the compile time of the fill kernels for windows — 101..104, 145..156 bases and the like — that no workload here has.)
constexpr int TILE_WIDTHS[] = {64, 60, 56};
constexpr int N_TILE_WIDTHS = sizeof(TILE_WIDTHS) / sizeof(TILE_WIDTHS[0]);

// Tile counts the kernels treat alike: up to 8 tiles (row-maximum reduction in registers, tile votes of the combine step),
// up to 16 (the WIDE reduction, the 16-bit tile sets of a PairState), up to 64 (minimal replay), up to 255 (tile indices are bytes, 255 = none:
// the longest window of the 16-bit kernels, 16320 bases, is 255 tiles of 64) and beyond.
constexpr int tile_count_class(int tiles) { return tiles <= 8 ? 0 : tiles <= 16 ? 1 : tiles <= 64 ? 2 : tiles <= 255 ? 3 : 4; }
constexpr int tiles_of(int len, int wt) { return (len + wt - 1) / wt; }

// The width in use for an upload whose widest window has max_window bases: the built width with the fewest swept columns
// (ties: the wider one, i.e. fewer tiles).  Where that width would move the window into another class of tile counts than
// 64-column tiles do (450 bases: eight tiles of 64, but nine of 52 or 56), the upload keeps 64.
constexpr int pick_tile_width(int max_window)
{
    if (max_window <= 0) return TILE_W;
    int best = TILE_W, best_cols = tiles_of(max_window, TILE_W) * TILE_W;
    for (int k = 0; k < N_TILE_WIDTHS; ++k) {
        const int wt = TILE_WIDTHS[k], cols = tiles_of(max_window, wt) * wt;
        if (cols < best_cols) { best = wt; best_cols = cols; }
    }
    if (tile_count_class(tiles_of(max_window, best)) != tile_count_class(tiles_of(max_window, TILE_W))) return TILE_W;
    return best;
}
constexpr bool is_tile_width(int wt)
{
    for (int k = 0; k < N_TILE_WIDTHS; ++k)
        if (TILE_WIDTHS[k] == wt) return true;
    return false;
}

static_assert(pick_tile_width(389) == 56 && pick_tile_width(390) == 56 && pick_tile_width(392) == 56, "seven tiles of 56");
static_assert(pick_tile_width(590) == 60 && pick_tile_width(448) == 64 && pick_tile_width(450) == 60, "");
static_assert(pick_tile_width(16320) == 64 && tiles_of(15300, pick_tile_width(15300)) <= 255, "tile indices fit a byte");

}  // namespace dsa
