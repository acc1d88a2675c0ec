// kernels_update.h -- writes of LISTED rows (wdbx_index_set_rows_at, wdbx_index_remove_rows): the scatter of a call's rows to
// their places, the refresh of every derived copy for exactly those rows, and the int8 groups they touch.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.
//
// Every kernel here walks LIST POSITIONS with the frame of the range quantisers -- one wave per row, four waves per workgroup,
// grid-stride, the row number wave-uniform -- and calls the per-row function the range kernel of the same copy calls
// (row_sqnorm, row_piece_to_bf16, row_to_u8, row_to_u6, row_to_u42, group_to_i8g, normalize_row), so a listed row's bytes are
// what the range kernel over [r, r + 1) writes.  The list is strictly increasing (host_update.h), so no two waves share a row
// and no two workgroups share a group: no atomics.

// ------------------------------------------------------------------------------------------------
// scatter: list position i0 + i takes row i of src ([n, dim], tight) at the row pitch, the pad elements zero (what copy_padded
// leaves), then normalize_rows_kernel's arithmetic on the stored row when asked.  src == nullptr: the row becomes the NaN
// tombstone of a removed row (quiet NaN, 0x7FC00000, in its dim elements; pads zero) and nothing is read.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void update_scatter_kernel(const float* src, const uint32_t* list, u64 i0, u64 n, uint32_t dim,
                                                             uint32_t pitch, float* rows, int normalize) {
  const int lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (u64)gridDim.x * 4;
  for (u64 i = wave; i < n; i += nw) {
    const u64 r = (u64)__builtin_amdgcn_readfirstlane((int)list[i0 + i]) & 0xFFFFFFFFull;
    float* p = rows + r * pitch;
    const float* from = src ? src + i * dim : nullptr;
    for (uint32_t c = lane; c < pitch; c += 64) p[c] = c < dim ? (from ? from[c] : __uint_as_float(0x7FC00000u)) : 0.f;
    if (normalize) normalize_row(p, pitch, lane);  // (a lane reads back its own stores only)
  }
}

// workgroups of an update_scatter_kernel / update_refresh_kernel launch over `rows` list positions: four waves = four rows each
static inline uint32_t update_rows_grid(uint64_t rows) { return (uint32_t)std::min<uint64_t>((rows + 3) / 4, 65536); }

// ------------------------------------------------------------------------------------------------
// refresh: every derived per-row copy of the listed rows in ONE launch.  A copy covers rows [0, its coverage); the list is
// sorted, so the listed rows it covers are the list's first n_* positions (0: the copy does not exist).  A wave takes a list
// position, reads the row once from HBM (the later bodies hit the cache) and feeds every copy whose count its position is
// below: wave-uniform branches.
// ------------------------------------------------------------------------------------------------
struct UpdateArgs {
  const float* rows;
  const uint32_t* list;
  uint32_t dim, pitch;
  uint32_t n_cn, n_16, n_8, n_6, n_42;  // list positions below each copy's coverage
  float* cn;
  __bf16* rows16;
  uint32_t pitch16;
  uint8_t* rows8;
  uint32_t pitch8;
  float* scale8;
  uint32_t units6;
  uint32_t* codes6;
  f2v* sa6;
  uint32_t units42, lpitch42;
  uint32_t* h42;
  f2v* sa42;
  uint32_t* lrec42;
};

__global__ __launch_bounds__(256) void update_refresh_kernel(UpdateArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t n = max(max(max(a.n_cn, a.n_16), max(a.n_8, a.n_6)), a.n_42);
  const u64 wave = (u64)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (u64)gridDim.x * 4;
  for (u64 i = wave; i < n; i += nw) {
    const u64 r = (u64)__builtin_amdgcn_readfirstlane((int)a.list[i]) & 0xFFFFFFFFull;
    const float* p = a.rows + r * a.pitch;
    if (i < a.n_cn) {
      const float s = row_sqnorm((const f4*)p, a.pitch / 4, lane);
      if (lane == 0) a.cn[r] = s;
    }
    if (i < a.n_16)
      for (uint32_t c = (uint32_t)lane * 8; c < a.pitch16; c += 512) row_piece_to_bf16(a.rows, r, c, a.pitch, a.rows16, a.pitch16);
    if (i < a.n_8) row_to_u8(p, r, a.dim, a.rows8, a.pitch8, a.scale8, lane);
    if (i < a.n_6) row_to_u6(p, r, a.dim, a.units6, a.codes6, a.sa6, lane);
    if (i < a.n_42) row_to_u42(p, r, a.dim, a.units42, a.h42, a.sa42, a.lrec42, a.lpitch42, lane);
  }
}

// ------------------------------------------------------------------------------------------------
// the int8 groups: a group's scale depends on all 64 of its rows, so the copy takes the DISTINCT groups of the list (host_update.h),
// one workgroup per listed group, rows_to_i8g_kernel's body and its n_rows.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rows_to_i8g_list_kernel(const float* rows, const uint32_t* group_list, u64 n_groups, u64 n_rows,
                                                               uint32_t dim, uint32_t pitch, int8_t* out, uint32_t pitch8, f4* groups,
                                                               u64* gbad) {
  __shared__ float red[4][4];
  __shared__ uint32_t redbad[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u64 gi = blockIdx.x; gi < n_groups; gi += gridDim.x)
    group_to_i8g(rows, (u64)group_list[gi], n_rows, dim, pitch, out, pitch8, groups, gbad, red, redbad, lane, wave);
}

// workgroups of a rows_to_i8g_list_kernel launch over `groups` listed groups: one each, as the range form
static inline uint32_t rows_to_i8g_list_grid(uint64_t groups) { return rows_to_i8g_grid(groups); }
