// Partition's overlap-tile geometry (lib/transforms.py:508-649), shared by the tiling kernels (datapath.hip) and the blending kernels (blend.hip).
#pragma once
#include "common.h"

struct TileGeom { int D, H, W; int tz, ty, tx; int oz, oy, ox; int gz, gy, gx; };   // volume, tile, overlap, tile grid (numpy order z, y, x)

static inline int tile_geom(TileGeom& g, int D, int H, int W, const int* tile3, const int* overlap3) {
    g.D = D; g.H = H; g.W = W; g.tz = tile3[0]; g.ty = tile3[1]; g.tx = tile3[2]; g.oz = overlap3[0]; g.oy = overlap3[1]; g.ox = overlap3[2];
    const int ez = g.tz - 2 * g.oz, ey = g.ty - 2 * g.oy, ex = g.tx - 2 * g.ox;
    if (D <= 0 || H <= 0 || W <= 0 || ez <= 0 || ey <= 0 || ex <= 0 || g.oz < 0 || g.oy < 0 || g.ox < 0) return DA_ERR_BADARG;
    g.gz = (D + ez - 1) / ez; g.gy = (H + ey - 1) / ey; g.gx = (W + ex - 1) / ex;
    return 0;
}
