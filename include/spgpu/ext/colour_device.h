#pragma once
/*
 * Multicolour ordering on CSR arrays, in HBM: a colouring of the adjacency graph with fixed priorities, the rows listed colour by
 * colour, and the symmetric permutation B = A(order, order) (the reference colours nothing and permutes no CSR matrix, and neither
 * did this library).
 *
 * NEW: the level-scheduled calls of spgpu/ext/trsv_device.h and spgpu/ext/ilu0_device.h run one launch per level, and the number
 * of levels is a property of the row order the caller holds: 3(n - 1) + 1 for the 7-point matrix of an n^3 grid in its natural
 * order.  Rows of one colour do not depend on each other, so on B the Plans that already exist find about as many levels as there
 * are colours.  Correctness of a solve never rests on the colouring: the Plans still derive the levels from the stored
 * dependencies.  A poor colouring costs levels, not answers.  A multicolour order usually costs a preconditioned solver
 * iterations; tools/multicolour_amd.c prints both sides of that trade.  spgpu/ext/sweep_device.h relaxes on A itself with this
 * colouring, one launch per colour, and there the colouring does carry correctness: its Plan checks it.
 *
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.
 *
 * THE CONTRACT
 * Matrix
 *   - one square CSR matrix of rowsCount rows with int indices and baseIndex 0 or 1;
 *   - columns need not ascend, a column may be stored twice, a row may lack its diagonal and a row may be empty.
 * Colouring (spgpuCsrColourDevice)
 *   - N(i) is the set of the columns j != i of the stored entries of row i;
 *   - the priority of node i is the tuple (hash(i), i), ordered lexicographically, with hash(i) = lowbias32(i) >> 1, where
 *     lowbias32(x) is x ^= x>>16; x *= 0x7FEB352D; x ^= x>>15; x *= 0x846CA68B; x ^= x>>16 on 32-bit unsigned words, exactly as in
 *     spgpu/ext/aggregate_device.h;
 *   - all nodes start uncoloured, with colour -1;
 *   - a round is synchronous and goes from buffer to buffer: c0 is the colouring at the start of the round.  An uncoloured i is
 *     ready if every j in N(i) has c0[j] >= 0 or has a smaller tuple than i.  A ready i takes the smallest c >= 0 that is not c0[j]
 *     for any j in N(i).  Every other node keeps c0[i];
 *   - rounds repeat until no node is uncoloured.  The uncoloured node with the largest tuple is always ready, so there are at most
 *     rowsCount rounds; *roundsCount receives the number of rounds, *coloursCount receives 1 + the largest colour;
 *   - colourOf[i], i < rowsCount, is 0-based whatever baseIndex is;
 *   - for a structurally symmetric pattern the result is a proper colouring (no stored off-diagonal entry joins two nodes of one
 *     colour) with at most 1 + the largest degree colours, and it is the one a sequential greedy pass in descending tuple order
 *     gives: two adjacent nodes are never ready in the same round, and a node's colour depends only on neighbours with larger
 *     tuples;
 *   - for an unsymmetric pattern the rounds are the definition.  Node j may then take, in the same round or later, the colour of a
 *     node i that stores no entry (i, j): the colouring need not be proper for the symmetrised graph, which costs levels
 *     afterwards, never a wrong solve;
 *   - AND, OR and "lowest zero bit" are exact, so no result depends on scheduling, on the kernel shape or on the grid, a repeated
 *     call gives the same bytes, and numpy can restate them (spgpu_amd.formats.csr_colour): the tests compare bytes.  The only
 *     atomics are integer: the count of the nodes still uncoloured and the running maximum colour; no floating-point atomics are
 *     used;
 *   - the call synchronises the stream about once per round (it returns host data) and cannot be captured;
 *   - `work` is caller-provided scratch of spgpuCsrColourWorkBytes(rowsCount) bytes, 256-byte aligned -- about 16 bytes per row,
 *     with no share of the entries.  It may be freed once the call has returned.
 * Refusal: SPGPU_UNSUPPORTED from the colouring with *coloursCount = 0 and *roundsCount = 0, reported after the first round's
 * synchronise with nothing read or written out of bounds; colourOf then has no defined content
 *   - an entry with a column outside [baseIndex, baseIndex + rowsCount).  The offending entry is clamped out (it is no neighbour)
 *     and a flag is raised, as the Plan of spgpu/ext/trsv_device.h does.
 * Order (spgpuCsrColourOrderDevice)
 *   - order[k], k < rowsCount, lists the 0-based rows by (colour, row) ascending; inverse[order[k]] = k;
 *   - colourPtr[c] is the number of rows of colours < c, for c <= coloursCount: coloursCount + 1 ints, nothing behind them is
 *     touched.  The rows of colour c are order[colourPtr[c] .. colourPtr[c + 1]);
 *   - coloursCount is the colouring's count; every colourOf[i] lies in [0, coloursCount);
 *   - the sort is one stable split per bit of coloursCount - 1 (flag, scan, scatter, one writer per position);
 *   - asynchronous, returns no host data, keeps no state and can be captured into a HIP graph;
 *   - `work` is spgpuCsrColourWorkBytes(rowsCount) bytes, 256-byte aligned; the call may share the colouring's.
 * Symmetric permutation (spgpuCsrPermuteDevice)
 *   - B = A(order, order): row k of B is row order[k] of A, and a stored column j becomes inverse[j - baseIndex] + baseIndex;
 *   - bRowPtr[k], k <= rowsCount, is the exclusive scan of the gathered row lengths, plus baseIndex; B has as many stored entries
 *     as A, so bColIndices and bValues are as long as A's;
 *   - a row's entries are written in ascending new column, entries with equal columns in A's storage order.  So a matrix without
 *     repeated columns comes out strictly ascending, which is what the Plan of spgpu/ext/ilu0_device.h demands;
 *   - the place of an entry is its rank among the entries of its row, counted entry against entry: the work is quadratic in the row
 *     length.  This is set-up code for rows of tens to hundreds of entries;
 *   - values are moved as 4-, 8- or 16-byte words: valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE, and
 *     -0.0 and NaN payloads survive; anything else returns SPGPU_UNSUPPORTED before a launch;
 *   - asynchronous, keeps no state and can be captured; every output byte has one writer; a call replayed after aValues changed
 *     in place gives the new coefficients;
 *   - B may not overlap A;
 *   - the call trusts order / inverse to be a permutation and its inverse, and the columns to lie inside the matrix: it is meant
 *     for a matrix the colouring accepted, as the solve of spgpu/ext/trsv_device.h trusts its Plan;
 *   - `work` is spgpuCsrPermuteWorkBytes(rowsCount) bytes, 256-byte aligned -- about 8 bytes per row.
 * Degenerate inputs
 *   - rowsCount <= 0: every call returns SPGPU_SUCCESS with nothing launched; the colouring sets both counts to 0;
 *   - a null output, a null input where it is read, or a null `work` with rows to do: SPGPU_UNSUPPORTED before a launch (the
 *     colouring sets both counts to 0).
 * State
 *   - no call allocates or keeps state; no kernel waits for another workgroup: rounds, splits and passes are ordered by stream order
 *     between launches, nothing else.
 *
 * A multicolour order for a matrix in HBM (A in CSR, fp64), and a solve on it:
 *
 *     spgpuCsrColourDevice(h, &colours, &rounds, colourOf, rows, aPtr, aIdx, base, work);
 *     spgpuCsrColourOrderDevice(h, order, inverse, colourPtr, rows, colours, colourOf, work);
 *     spgpuCsrPermuteDevice(h, bPtr, bIdx, bVal, rows, order, inverse, aPtr, aIdx, aVal, base, SPGPU_TYPE_DOUBLE, permuteWork);
 *     (the Plans of spgpu/ext/trsv_device.h or spgpu/ext/ilu0_device.h on B: about `colours` levels)
 *     spgpuDgath(h, bp, rows, order, 0, b);        b on the new order: bp[k] = b[order[k]]
 *     (solve B * xp = bp)
 *     spgpuDgath(h, x, rows, inverse, 0, xp);      x back on the old order: x[i] = xp[inverse[i]]
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCsrColourDevice and spgpuCsrColourOrderDevice; monotone in
 * rowsCount, and the same for rowsCount <= 0 as for rowsCount == 0. */
size_t spgpuCsrColourWorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  The colours of the adjacency graph.  Synchronises the stream about once per round
 * (returns host data).  Writes colourOf[rowsCount]. */
spgpuStatus_t spgpuCsrColourDevice(spgpuHandle_t handle, __host int* coloursCount, __host int* roundsCount, __device int* colourOf,
                                   int rowsCount, const __device int* rowPtr, const __device int* colIndices, int baseIndex,
                                   __device void* work);

/* NEW (no counterpart in the reference).  order[rowsCount], inverse[rowsCount], colourPtr[coloursCount + 1].  Asynchronous, no
 * state. */
spgpuStatus_t spgpuCsrColourOrderDevice(spgpuHandle_t handle, __device int* order, __device int* inverse, __device int* colourPtr,
                                        int rowsCount, int coloursCount, const __device int* colourOf, __device void* work);

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCsrPermuteDevice; monotone in rowsCount, and the same for
 * rowsCount <= 0 as for rowsCount == 0. */
size_t spgpuCsrPermuteWorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  B = A(order, order): bRowPtr[rowsCount + 1], bColIndices and bValues as long as A's.
 * Asynchronous, no state. */
spgpuStatus_t spgpuCsrPermuteDevice(spgpuHandle_t handle, __device int* bRowPtr, __device int* bColIndices, __device void* bValues,
                                    int rowsCount, const __device int* order, const __device int* inverse,
                                    const __device int* aRowPtr, const __device int* aColIndices, const __device void* aValues,
                                    int baseIndex, spgpuType_t valuesType, __device void* work);

#ifdef __cplusplus
}
#endif
