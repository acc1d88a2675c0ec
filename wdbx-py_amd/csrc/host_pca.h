// host_pca.h -- the device-free host side of wdbx_index_moments and wdbx_index_project: argument
// checks, the padded dimension, the tile groups of the scatter pass (which 32 x 32 tiles of the upper triangle, which wave,
// which staged column blocks), their LDS, the row ranges and their partials, the column-sum ranges, and the grids.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/pca_harness.cpp (plain g++ in the CPU suite,
// tests/test_pca_host.py).  No HIP, no kernel types in here.  The group and tile functions are constexpr: the kernels of
// kernels_pca.h call the same ones, so the device walks exactly the tiles the plan (and its test) describe.
#pragma once

#include <cstddef>
#include <cstdint>

constexpr int PCA_MAX_COMPONENTS = 32;  // = WDBX_MAX_COMPONENTS: one 32-wide MFMA block of basis vectors
constexpr int PCA_MAX_DIM = 4096;       // the scatter matrix is served up to this dimension (128 MiB of float64 on the host)
constexpr int PCA_CHUNK_ROWS = 32;      // stored rows staged per chunk = 16 row pairs of v_mfma_f32_32x32x2_f32
constexpr int PCA_WAVES = 8;            // waves of a scatter workgroup: two per SIMD, one workgroup per CU
constexpr int PCA_WAVE_TILES = 10;      // tiles a wave holds at most: 160 accumulator registers of its 256 (12 tiles leave the
                                        // loader and the fragments too few: the compiler then goes to scratch)
constexpr int PCA_SIDE_SINGLE = 12;     // a triangle of up to 12 x 12 blocks is ONE group (78 tiles, 10 per wave)
constexpr int PCA_SIDE_MULTI = 8;       // otherwise square super-tiles of 8 x 8 blocks (64 tiles, 8 per wave; 16 staged blocks)
// one workgroup per CU may take this much of the CU's 160 KiB
constexpr size_t PCA_LDS_LIMIT = 144 * 1024;
// all partials of one call stay within this much scratch; more than KEEP is released when the call ends (as assign's)
constexpr size_t PCA_PARTIALS_BUDGET = 256u << 20;
constexpr size_t PCA_PARTIALS_KEEP = 64u << 20;
// the projection: a workgroup's 4 waves take 32 stored rows each, K in chunks of 32 floats
constexpr int PCA_PROJECT_TILE_ROWS = 128;
constexpr int PCA_PROJECT_BK = 32;
constexpr int PCA_PROJECT_LD = PCA_PROJECT_BK + 1;  // padded LDS row (floats): conflict-free ds_read_b32 down a column

// (always inlined: in the kernels the group and its tiles must stay in registers, not behind calls with the group on the stack)
#define PCA_FN constexpr __attribute__((always_inline)) inline
PCA_FN int pca_min(int a, int b) { return a < b ? a : b; }
PCA_FN int pca_blocks(int dim) { return (dim + 31) / 32; }  // nb: 32-column blocks, dp = 32 nb

enum PcaCheck { PCA_OK = 0, PCA_BAD_COMPONENTS, PCA_NULL_BASIS, PCA_NULL_OUTPUT, PCA_DIM_TOO_LARGE, PCA_BAD_CENTER };

static inline PcaCheck moments_validate(int center, bool any_output, bool want_scatter, int dim) {
  if (center != 0 && center != 1) return PCA_BAD_CENTER;
  if (!any_output) return PCA_NULL_OUTPUT;
  if (want_scatter && dim > PCA_MAX_DIM) return PCA_DIM_TOO_LARGE;
  return PCA_OK;
}
static inline PcaCheck project_validate(int m, bool have_basis, bool have_out) {
  if (m < 1 || m > PCA_MAX_COMPONENTS) return PCA_BAD_COMPONENTS;
  if (!have_basis) return PCA_NULL_BASIS;
  if (!have_out) return PCA_NULL_OUTPUT;
  return PCA_OK;
}

// blocks per side of a tile group: the whole triangle when it has at most PCA_SIDE_SINGLE blocks a side (and nothing smaller
// is forced), else at most PCA_SIDE_MULTI -- an off-diagonal 8 x 8 group is 64 tiles, 8 per wave, and stages 16 column blocks
PCA_FN int pca_group_side(int nb, int forced) {
  const int g = forced > 0 ? forced : PCA_SIDE_SINGLE;
  if (g >= nb && nb <= PCA_SIDE_SINGLE) return nb;
  return pca_min(g, PCA_SIDE_MULTI);
}
PCA_FN int pca_group_count(int nb, int side) {
  const int ns = (nb + side - 1) / side;
  return ns * (ns + 1) / 2;
}

// One tile group: super-tile (si, sj), si <= sj, of the upper triangle.  Its tiles are blocks (I, J) with I in [i0, i0 + ni),
// J in [j0, j0 + nj) and, in a diagonal group (si == sj), J >= I.  They are numbered row-major (I ascending, then J) and wave
// w takes the consecutive run [w per_wave, (w + 1) per_wave): mostly one I, so mostly one A fragment.
// Staged column blocks, in LDS order: the I blocks, then (off-diagonal groups) the J blocks.
struct PcaGroup {
  int si, sj, i0, ni, j0, nj, tiles, per_wave, staged;
};
PCA_FN PcaGroup pca_group(int nb, int side, int g) {
  const int ns = (nb + side - 1) / side;
  int si = 0, rem = g;
  while (rem >= ns - si) {
    rem -= ns - si;
    ++si;
  }
  PcaGroup G = {};
  G.si = si;
  G.sj = si + rem;
  G.i0 = G.si * side;
  G.ni = pca_min(side, nb - G.i0);
  G.j0 = G.sj * side;
  G.nj = pca_min(side, nb - G.j0);
  G.tiles = G.si == G.sj ? G.ni * (G.ni + 1) / 2 : G.ni * G.nj;
  G.per_wave = (G.tiles + PCA_WAVES - 1) / PCA_WAVES;
  G.staged = G.si == G.sj ? G.ni : G.ni + G.nj;
  return G;
}
// tile q of the group -> its staged blocks: a = the A operand's (block I), b = the B operand's (block J), both LDS positions
PCA_FN void pca_tile_staged(const PcaGroup& G, int q, int* a, int* b) {
  if (G.si != G.sj) {
    *a = q / G.nj;
    *b = G.ni + q % G.nj;
    return;
  }
  int i = 0;
  while (q >= G.ni - i) {
    q -= G.ni - i;
    ++i;
  }
  *a = i;
  *b = i + q;
}
// the column block a staged position holds
PCA_FN int pca_staged_block(const PcaGroup& G, int s) { return s < G.ni ? G.i0 + s : G.j0 + (s - G.ni); }
// floats of a staged row: the group's blocks, padded so that two consecutive rows start 32 banks apart (a fragment read takes
// 32 floats of each of two consecutive rows)
PCA_FN int pca_lds_row(int staged) { return staged * 32 + ((staged & 1) ? 0 : 32); }
PCA_FN size_t pca_lds_bytes(int staged) { return (size_t)2 * PCA_CHUNK_ROWS * pca_lds_row(staged) * sizeof(float); }

struct PcaPlan {
  int dp = 0, nb = 0;          // padded dimension = 32 nb
  int side = 0, groups = 0;    // blocks per side of a tile group; groups of the upper triangle
  int wave_tiles = 0;          // the most tiles any wave holds
  int staged = 0;              // the most column blocks any group stages
  int instance = 0;            // the kernel instance = tiles a wave's registers hold: 1, 2, 4, 6 or 8 (<= 16 staged blocks) or 10 (<= 12 staged blocks)
  size_t lds = 0;              // dynamic LDS of the scatter launch (the largest group's)
  uint32_t ranges = 0;         // P: row ranges = partials [P][dp][dp] fp32; grid = P x groups
  uint64_t range_rows = 0;     // L: rows of a range, a multiple of PCA_CHUNK_ROWS
  size_t partial_bytes = 0;
  uint32_t sum_ranges = 0;     // ranges of the column-sum pass, one wave each
  uint64_t sum_rows = 0;       // rows of a column-sum range
  uint32_t sum_grid = 0;       // = ceil(sum_ranges / 4)
  size_t sum_bytes = 0;        // sum_ranges * (pitch floats + one counter)
};

// forced_side = option moments_tiles_per_group, forced_ranges = option moments_partials (0: the plan's choice).
// with_scatter = false plans the column sums alone (any dimension).
static inline PcaPlan pca_plan(uint64_t n_rows, int dim, uint32_t pitch, int cu_count, int forced_side, int64_t forced_ranges,
                               bool with_scatter) {
  PcaPlan p;
  const uint64_t cus = (uint64_t)(cu_count > 0 ? cu_count : 1);
  p.nb = pca_blocks(dim);
  p.dp = 32 * p.nb;
  if (with_scatter) {
    p.side = pca_group_side(p.nb, forced_side);
    p.groups = pca_group_count(p.nb, p.side);
    for (int g = 0; g < p.groups; ++g) {
      const PcaGroup G = pca_group(p.nb, p.side, g);
      if (G.per_wave > p.wave_tiles) p.wave_tiles = G.per_wave;
      if (G.staged > p.staged) p.staged = G.staged;
    }
    p.instance = p.wave_tiles <= 2 ? p.wave_tiles : p.wave_tiles <= 8 ? (p.wave_tiles + 1) / 2 * 2 : PCA_WAVE_TILES;
    p.lds = pca_lds_bytes(p.staged);
    const uint64_t chunks = (n_rows + PCA_CHUNK_ROWS - 1) / PCA_CHUNK_ROWS;
    const uint64_t per = (uint64_t)p.dp * p.dp * sizeof(float);
    uint64_t R = forced_ranges > 0 ? (uint64_t)forced_ranges : (cus + p.groups - 1) / p.groups;  // one workgroup per CU
    const uint64_t fit = PCA_PARTIALS_BUDGET / per;
    if (R > fit) R = fit;
    if (R > chunks) R = chunks;
    if (R < 1) R = 1;
    const uint64_t cpr = chunks ? (chunks + R - 1) / R : 0;
    if (cpr) R = (chunks + cpr - 1) / cpr;  // (no empty range)
    p.ranges = (uint32_t)R;
    p.range_rows = cpr * PCA_CHUNK_ROWS;
    p.partial_bytes = (size_t)(R * per);
  }
  const uint64_t per_sum = (uint64_t)pitch * sizeof(float) + sizeof(uint32_t);
  uint64_t S = forced_ranges > 0 ? (uint64_t)forced_ranges : 8 * cus;
  if (S > PCA_PARTIALS_BUDGET / per_sum) S = PCA_PARTIALS_BUDGET / per_sum;
  if (S > n_rows) S = n_rows;
  if (S < 1) S = 1;
  p.sum_rows = n_rows ? (n_rows + S - 1) / S : 0;
  if (p.sum_rows) S = (n_rows + p.sum_rows - 1) / p.sum_rows;
  p.sum_ranges = (uint32_t)S;
  p.sum_grid = (uint32_t)((S + 3) / 4);
  p.sum_bytes = (size_t)(S * per_sum);
  return p;
}

// the projection: tiles of PCA_PROJECT_TILE_ROWS rows over a persistent grid, three workgroups a CU (their LDS allows it)
static inline size_t project_lds_bytes() {
  return (size_t)2 * (PCA_PROJECT_TILE_ROWS + 32) * PCA_PROJECT_LD * sizeof(float);
}
static inline uint32_t project_grid(uint64_t n_rows, int cu_count) {
  const uint64_t tiles = (n_rows + PCA_PROJECT_TILE_ROWS - 1) / PCA_PROJECT_TILE_ROWS;
  const uint64_t cap = (uint64_t)3 * (uint64_t)(cu_count > 0 ? cu_count : 1);
  return (uint32_t)(tiles < 1 ? 1 : tiles < cap ? tiles : cap);
}
