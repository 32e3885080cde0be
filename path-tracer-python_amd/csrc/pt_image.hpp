// pt_image.hpp — what the image kernels share (pt_denoise.hip,
// pt_reproject.hip, pt_validate.hip, the guide trace of pt_guide.hip, the flat
// kernels of pt_abi.hip): a pixel between its float4 and its math-header form, the block
// geometry of "one block per square tile on a 1-D grid", and the capped flat
// grid of the grid-stride kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "pt_denoise_math.hpp"

namespace ptmi {

__device__ __forceinline__ DnPx px_from4(float4 v) {
  DnPx p;
  p.r = v.x;
  p.g = v.y;
  p.b = v.z;
  p.v = v.w;
  return p;
}

__device__ __forceinline__ float4 px_to4(const DnPx& p) { return make_float4(p.r, p.g, p.b, p.v); }

// Guide pixel q of a guide image: two 16-B loads.
__device__ __forceinline__ DngG load_guide(const float4* __restrict__ guides, size_t q) {
  const float4 n = guides[2 * q], a = guides[2 * q + 1];
  DngG g;
  g.nx = n.x;
  g.ny = n.y;
  g.nz = n.z;
  g.z = n.w;
  g.ar = a.x;
  g.ag = a.y;
  g.ab = a.z;
  g.hit = a.w;
  return g;
}

// One block of TILE x TILE lanes per TILE x TILE pixel tile, tiles in row-major
// order over a 1-D grid (an image of 1 x 2^31-1 pixels has more tile rows than
// a grid's y extent). TILE is a power of two.
constexpr int kImgTile = 16;  // the filter passes and the reprojection
constexpr int kImgBlock = kImgTile * kImgTile;

inline int32_t image_tiles_x(int32_t width, int32_t tile) { return (width + tile - 1) / tile; }

// At most 2^31-1 pixels / TILE + one partial tile per row: below 2^32 blocks.
inline dim3 image_tile_grid(int32_t width, int32_t height, int32_t tile) {
  return dim3((unsigned)((int64_t)image_tiles_x(width, tile) * ((height + tile - 1) / tile)));
}

struct TileXY {
  int32_t x0, y0;  // the tile's origin
  int32_t x, y;    // this lane's pixel (may lie outside the image)
};

template <int TILE>
__device__ __forceinline__ TileXY tile_xy(int32_t tiles_x) {
  const int32_t ty = (int32_t)(blockIdx.x / (uint32_t)tiles_x), tx = (int32_t)(blockIdx.x - (uint32_t)ty * tiles_x);
  TileXY t;
  t.x0 = tx * TILE;
  t.y0 = ty * TILE;
  t.x = t.x0 + (int32_t)(threadIdx.x & (TILE - 1));
  t.y = t.y0 + (int32_t)(threadIdx.x / TILE);
  return t;
}

// One thread per element in grid-stride loops: at most 4096 blocks.
inline dim3 capped_grid(int64_t n, int block) {
  const int64_t g = (n + block - 1) / block;
  return dim3((unsigned)(g > 4096 ? 4096 : g));
}

}  // namespace ptmi
