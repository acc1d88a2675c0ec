"""The selection plan as the four enqueue functions of host_index.h spelled it out before host_selection.h existed: a
transcription of THOSE expressions (not of the header), with their 32-bit unsigned arithmetic made explicit.  The CPU test
compares the header against it field by field, the GPU test the capacities the library reports."""
import math
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wdbx-py_amd" / "csrc"
M32 = 0xFFFFFFFF


def _const(header, name):
    m = re.search(r"constexpr int [^;]*\b%s = (\d+)" % name, (CSRC / header).read_text())
    return int(m.group(1))


GB_M = _const("kernels_tiles.h", "GB_M")       # rows of an exact fp32 tile
GW_M = _const("kernels_tiles.h", "GW_M")       # rows of a bf16 tile
G8_ROWS = _const("kernels_tiles8.h", "G8_ROWS")  # rows of an int8 tile
MAX_K = int(re.search(r"#define WDBX_MAX_K (\d+)", (ROOT / "include" / "wdbx_hip.h").read_text()).group(1))

# (tile rows, lower bounds per tile and query, divisor grows with k, capacity factor) of the four callers
U8 = (256, 4, True, 32)
U6 = (256, 4, True, 256)
LEGACY_FP32 = (GB_M, GB_M // 64, False, 8)
LEGACY_BF16 = (GW_M, GW_M // 64, True, 32)
INT8 = (G8_ROWS, G8_ROWS // 32, True, 32)
CALLERS = {"u8": U8, "u6": U6, "fp32": LEGACY_FP32, "bf16": LEGACY_BF16, "int8": INT8}


def div_of(div_option, k, k_scaled):
    # opt_gemm_sample_div > 0 ? (uint32_t)opt : [bf16 ?] std::min(32u, std::max(4u, 1024u / (uint32_t)k)) [: 32u]
    if div_option > 0:
        return div_option & M32
    return min(32, max(4, 1024 // k)) if k_scaled else 32


def _unclamped(n_rows, tile_rows, rw, k, div):
    tiles = ((n_rows + tile_rows - 1) // tile_rows) & M32
    return tiles, max(tiles // div, ((8 * k + rw - 1) & M32) // rw)


def _finish(tiles, sample_tiles, rw, k, factor):
    sample_tiles = max(1, min(sample_tiles, tiles))
    expect = k * (tiles // sample_tiles + 1)
    bounds = (rw * sample_tiles) & M32
    return {"tiles": tiles, "sample_tiles": sample_tiles, "stride": tiles // sample_tiles, "bounds": bounds, "expect": expect,
            "too_small": bounds < k, "cap": min(max(4096, expect * factor), 1 << 22)}


def plan(n_rows, tile_rows, rw, k, div_option, k_scaled, factor):
    div = div_of(div_option, k, k_scaled)
    tiles, sample_tiles = _unclamped(n_rows, tile_rows, rw, k, div)
    return dict(_finish(tiles, sample_tiles, rw, k, factor), div=div)


def masked_sample(n_rows, tile_rows, rw, k, div_option, allowed):
    """sample_for(true, allowed) of enqueue_search_gemm8: the tiles a masked call (or block) samples."""
    tiles, sample_tiles = _unclamped(n_rows, tile_rows, rw, k, div_of(div_option, k, True))
    if allowed > 16384:
        f = allowed / n_rows if n_rows else 0.0
        if f > 0.0:
            pv = 1.0 - math.pow(1.0 - min(f, 1.0), 32.0)
            scaled = float(sample_tiles) * min(1.0 / f, 8.0)
            vouch = (8.0 * k) / (rw * max(pv, 1e-9))
            sample_tiles = int(min(math.ceil(max(scaled, vouch)), float(tiles)))
    return max(1, min(sample_tiles, tiles))


def masked_plan(n_rows, k, div_option, allowed, small_class=0):
    """... and what follows from it on the int8 tiles: stride, bounds, expected rows and the candidate capacity (a mask of
    at most 16 384 rows -- small_class -- gets room for all its rows)."""
    tile_rows, rw, _, factor = INT8
    tiles, _ = _unclamped(n_rows, tile_rows, rw, k, 1)
    p = _finish(tiles, masked_sample(n_rows, tile_rows, rw, k, div_option, allowed), rw, k, factor)
    p["cap"] = max(p["cap"], small_class)
    return p


def pair_cap(expect, nwaves):
    # (uint32_t)std::min<uint64_t>(std::max<uint64_t>(16384, (uint64_t)GB_N * expect * 16 / nwaves), 1u << 16), GB_N = 256
    return min(max(16384, 256 * expect * 16 // nwaves), 1 << 16)


def shadow_over_1gib(n_rows, u8_pitch):
    # the sites tested (uint64_t)n * pitch <= (1ull << 30) for "not over"
    return not (n_rows * u8_pitch <= (1 << 30))
