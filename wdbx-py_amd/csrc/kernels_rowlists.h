// kernels_rowlists.h -- exact scores among LISTED rows with one row list PER QUERY (wdbx_index_search_row_lists): one
// workgroup per work item of host_rowlists.h, a (chunk of one list, block of that list's queries) pair.  The scores are
// subset_kernel's (the frame of kernels_rowblock.h), so an answer equals wdbx_index_search_rows' bit for bit.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_subset.h); not a standalone header.

struct RowListsArgs {
  const f4* rows;             // [n_rows, pitch4] quads
  const f4* queries;          // [slots, pitch4] the round's queries in slot order
  const uint32_t* ids;        // the call's lists back to back, each strictly increasing (validated on the host)
  const RowListsItem* items;  // [gridDim.x] the round's work items
  u64* keys;                  // [slots][stride]: entry i of a slot = the key of row i of its list
  uint64_t stride;
  uint32_t pitch4;
};

// Grid: x = work items.  Wave w of the workgroup takes the chunk's listed rows w, w + 4, ... with U rows' loads in flight;
// every fetched row is scored against the block's QB queries (in registers for the whole item when NI > 0).  A score is
// wave-uniform (the xor tree is symmetric), lane 0 writes its key.  A short block's idle query slots repeat the block's last
// query and write nothing.  No LDS, no list, no atomic: ranking is merge_kernel's, over the slot's keys as unsorted candidates.
template <int METRIC, int QB, int NI>
__global__ __launch_bounds__(256) void rowlists_kernel(RowListsArgs a) {
  constexpr int U = row_block_u(NI), NR = row_block_nr(NI);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)lane;
  const RowListsItem it = a.items[blockIdx.x];  // (uniform over the workgroup)
  const uint32_t* ids = a.ids + it.first;
  const f4* qp[QB];
  f4 q[QB][NR];
#pragma unroll
  for (int b = 0; b < QB; ++b) {
    qp[b] = a.queries + (size_t)(it.slot + min((uint32_t)b, it.nq - 1)) * a.pitch4;
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      q[b][t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) q[b][t] = qp[b][j + (uint32_t)t * 64];
    }
  }
  u64* const out = a.keys + (size_t)it.slot * a.stride + it.offset;
  for (uint32_t cur = (uint32_t)wave; cur < it.n; cur += U * 4) {
    f4 c[U][NR];
    uint32_t row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t idx = cur + (uint32_t)u * 4;
      row[u] = ids[min(idx, it.n - 1)];  // (past the end: the chunk's last row again, dropped below)
      const f4* cp = a.rows + (size_t)row[u] * a.pitch4;
#pragma unroll
      for (int t = 0; t < NR; ++t) {
        c[u][t] = f4{0.f, 0.f, 0.f, 0.f};
        if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) c[u][t] = ld16<true>(cp + j + (uint32_t)t * 64);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t idx = cur + (uint32_t)u * 4;
      const bool live = idx < it.n;  // (wave-uniform)
      float s[QB];
      exact_score_block<METRIC, QB, NI>(c[u], a.rows + (size_t)row[u] * a.pitch4, q, qp, a.pitch4, j, s);
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        const u64 mine = row_key(s[b], row[u]);
        if (lane == 0 && live && (uint32_t)b < it.nq) out[(size_t)b * a.stride + idx] = mine;
      }
    }
  }
}

typedef void (*rowlists_fn)(RowListsArgs);

// qb as rowlists_plan (host_rowlists.h) chooses it: 1 or 8; null for anything else
static rowlists_fn pick_rowlists(int metric, int qb, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> rowlists_fn {
    constexpr int NI = decltype(ni)::value;
    const bool l2 = metric == WDBX_METRIC_L2;
    if (qb == 1) return l2 ? rowlists_kernel<WDBX_METRIC_L2, 1, NI> : rowlists_kernel<WDBX_METRIC_COSINE, 1, NI>;
    if (qb == ROWLISTS_QB) return l2 ? rowlists_kernel<WDBX_METRIC_L2, ROWLISTS_QB, NI> : rowlists_kernel<WDBX_METRIC_COSINE, ROWLISTS_QB, NI>;
    return nullptr;
  });
}
