"""The constants of the Level-1 dispatch (spgpu_amd/csrc/level1_grid.h, spgpu_internal.h) and the sizes at which its choices flip, stated once
for tests/test_gpu_level1_shapes.py (which runs them on the GPU) and tests/test_exact_ref.py (which checks on the CPU that the integer
inputs chosen for those sizes add exactly).  No torch, no library: importable everywhere."""

# ---- the constants of the dispatch, with the name that sets each (tests/test_level1_grid.py compares): a change there is a test to
# revisit here
THREADS = 256            # level1_grid.h     kL1Threads
UNROLL = 4               # level1_grid.h     kL1Unroll
MAP_MAX_BLOCKS = 16384   # level1_grid.h     kL1MaxBlocks (singleLaunchCap: axpbyGrid, mapGrid; axpbyDeviceGrid; sparseGrid uses 4 x this)
REDUCE_MAX_BLOCKS = 1024  # spgpu_internal.h  SPGPU_REDUCE_MAX_BLOCKS (blocks of one vector, and vectors of one pass: reduceGrid's cap)
NT_BYTES = 256 << 20     # level1_grid.h     kL1StreamedBytes: streamed bytes from which the non-temporal kernels run (beyondCache)
SIZEOF = {"S": 4, "D": 8, "C": 8, "Z": 16}
WIDE = {L: 16 // s for L, s in SIZEOF.items()}     # level1_grid.h     wideOf
TILE = THREADS * UNROLL                            # packs one block handles per trip
RAGGED = 1029                                      # one full tile of packs + 5 elements: a ragged last tile and a tail for every WIDE > 1


def n_past_map_cap(letter):
    """Smallest interesting n whose wide grid is capped: the cap's worth of tiles, one more tile, 5 more elements."""
    return MAP_MAX_BLOCKS * TILE * WIDE[letter] + RAGGED


def n_past_reduce_cap(letter):
    return REDUCE_MAX_BLOCKS * TILE * WIDE[letter] + RAGGED


def n_reduce_nt(letter):
    """nrm2 streams n * sizeof: the first n that is non-temporal, plus a ragged end (dot, 2 * n * sizeof, is then past it too)."""
    return NT_BYTES // SIZEOF[letter] + RAGGED


#: (seed of the dot / nrm2 pair, seed of the asum / amax vector) of the two large reduction tests
REDUCE_CAP_SEEDS = (41, 43)
REDUCE_NT_SEEDS = (51, 53)
