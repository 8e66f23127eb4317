/*
 * The way back out of the library's formats (spgpu/ext/to_csr_device.h), written against the C ABI only.
 * A small ragged CSR matrix (rows x cols, row i of (i * 7) % 23 entries, columns in no order, duplicates present) goes into
 * HELL in HBM with spgpuCsrToHellDevice and comes back with spgpuHellToCsrRowPtrDevice / spgpuHellToCsrDevice: the three
 * arrays must be the caller's, byte for byte (memcmp).  Then A^T is built from the stored HELL arrays
 * (spgpu/ext/transpose_device.h) and taken to CSR the same way: those are the CSC arrays of A, compared with a CSC built here
 * by a stable counting sort by column.
 *
 *   usage: to_csr_amd [rows=3000] [cols=2000]
 * Prints OK or MISMATCH for each leg; exits non-zero if a call fails or a leg differs.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/convert_device.h"
#include "spgpu/ext/csr_device.h"
#include "spgpu/ext/to_csr_device.h"
#include "spgpu/ext/transpose_device.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)

#define OK(call)                                                                          \
    do {                                                                                  \
        spgpuStatus_t s_ = (call);                                                        \
        if (s_ != SPGPU_SUCCESS) {                                                        \
            fprintf(stderr, "%s:%d: %s -> status %d\n", __FILE__, __LINE__, #call, s_);   \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)

static void* deviceAlloc(size_t bytes)
{
    void* p;
    CHECK(hipMalloc(&p, bytes ? bytes : 16));
    return p;
}

static void* deviceCopyOf(const void* host, size_t bytes)
{
    void* p = deviceAlloc(bytes);
    CHECK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    return p;
}

static int sameAsHost(const void* device, const void* host, size_t bytes)
{
    void* back = malloc(bytes ? bytes : 1);
    CHECK(hipMemcpy(back, device, bytes, hipMemcpyDeviceToHost));
    const int same = memcmp(back, host, bytes) == 0;
    free(back);
    return same;
}

/* HELL arrays in HBM -> CSR arrays in HBM; 1 if they equal the host arrays given */
static int hellToCsrEquals(spgpuHandle_t h, const double* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS,
                           int rows, int slots, int base, const int* wantPtr, const int* wantCols, const double* wantVals, int wantNnz)
{
    void* work = deviceAlloc(spgpuToCsrWorkBytes(rows));
    int* rowPtr = (int*)deviceAlloc(((size_t)rows + 1) * sizeof(int));
    int nnz = -1, longest = -1;
    OK(spgpuHellToCsrRowPtrDevice(h, rowPtr, &nnz, &longest, base, hackSize, hackOffsets, rS, NULL, rows, slots, work));
    int* cols = (int*)deviceAlloc((size_t)nnz * sizeof(int));
    double* vals = (double*)deviceAlloc((size_t)nnz * sizeof(double));
    OK(spgpuHellToCsrDevice(h, cols, vals, rowPtr, base, cM, rP, hackSize, hackOffsets, rS, NULL, rows, base, SPGPU_TYPE_DOUBLE));
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    const int same = nnz == wantNnz && sameAsHost(rowPtr, wantPtr, ((size_t)rows + 1) * sizeof(int)) &&
                     sameAsHost(cols, wantCols, (size_t)nnz * sizeof(int)) && sameAsHost(vals, wantVals, (size_t)nnz * sizeof(double));
    CHECK(hipFree(work));
    CHECK(hipFree(rowPtr));
    CHECK(hipFree(cols));
    CHECK(hipFree(vals));
    return same;
}

int main(int argc, char** argv)
{
    const int rows = argc > 1 ? atoi(argv[1]) : 3000;
    const int cols = argc > 2 ? atoi(argv[2]) : 2000;
    const int hackSize = 32, base = 1;
    if (rows < 1 || cols < 1 || rows > 10000000 || cols > 10000000) {
        fprintf(stderr, "usage: to_csr_amd [rows] [cols]\n");
        return 2;
    }

    /* the caller's CSR, base 1: columns by a multiplicative hash (unsorted, with repeats), values that name their entry */
    int* ptr = (int*)malloc(((size_t)rows + 1) * sizeof(int));
    ptr[0] = base;
    for (int i = 0; i < rows; ++i)
        ptr[i + 1] = ptr[i] + (int)(((long long)i * 7) % 23);
    const int nnz = ptr[rows] - base;
    int* ci = (int*)malloc((size_t)(nnz ? nnz : 1) * sizeof(int));
    double* cv = (double*)malloc((size_t)(nnz ? nnz : 1) * sizeof(double));
    for (int e = 0; e < nnz; ++e) {
        ci[e] = (int)(((unsigned)e * 2654435761u) % (unsigned)cols) + base;
        cv[e] = (double)e + 0.25;
    }

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS)
        return 2;

    /* CSR -> HELL in HBM */
    int* dPtr = (int*)deviceCopyOf(ptr, ((size_t)rows + 1) * sizeof(int));
    int* dCi = (int*)deviceCopyOf(ci, (size_t)nnz * sizeof(int));
    double* dCv = (double*)deviceCopyOf(cv, (size_t)nnz * sizeof(double));
    const int hacks = (rows + hackSize - 1) / hackSize;
    int* rS = (int*)deviceAlloc((size_t)rows * sizeof(int));
    int* hackOffsets = (int*)deviceAlloc((size_t)hacks * sizeof(int));
    void* planWork = deviceAlloc(spgpuCooConvertWorkBytes(rows, 0));
    int longest = 0, height = 0;
    OK(spgpuCsrRowLengthsDevice(h, rS, &longest, rows, dPtr, base));
    OK(spgpuHellPlanDevice(h, &height, hackOffsets, hackSize, rows, rS, planWork));
    const int slots = hackSize * height;
    double* cM = (double*)deviceAlloc((size_t)slots * sizeof(double));
    int* rP = (int*)deviceAlloc((size_t)slots * sizeof(int));
    CHECK(hipMemset(cM, 0, (size_t)slots * sizeof(double)));
    CHECK(hipMemset(rP, 0, (size_t)slots * sizeof(int)));
    OK(spgpuCsrToHellDevice(h, cM, rP, hackOffsets, hackSize, base, rows, dPtr, dCi, dCv, base, SPGPU_TYPE_DOUBLE, NULL));
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    printf("A: %d x %d, %d entries, longest row %d, %d HELL slots (hackSize %d)\n", rows, cols, nnz, longest, slots, hackSize);

    /* leg 1: HELL -> CSR gives the caller's arrays */
    const int leg1 = hellToCsrEquals(h, cM, rP, hackSize, hackOffsets, rS, rows, slots, base, ptr, ci, cv, nnz);
    printf("HELL -> CSR against the caller's CSR: %s\n", leg1 ? "OK" : "MISMATCH");

    /* the CSC of A on the host: a stable counting sort of the entries by column */
    int* cscPtr = (int*)calloc((size_t)cols + 1, sizeof(int));
    int* cscRows = (int*)malloc((size_t)(nnz ? nnz : 1) * sizeof(int));
    double* cscVals = (double*)malloc((size_t)(nnz ? nnz : 1) * sizeof(double));
    for (int e = 0; e < nnz; ++e)
        ++cscPtr[ci[e] - base + 1];
    for (int j = 0; j < cols; ++j)
        cscPtr[j + 1] += cscPtr[j];
    int* next = (int*)malloc(((size_t)cols + 1) * sizeof(int));
    memcpy(next, cscPtr, ((size_t)cols + 1) * sizeof(int));
    for (int i = 0; i < rows; ++i)
        for (int e = ptr[i] - base; e < ptr[i + 1] - base; ++e) {
            const int at = next[ci[e] - base]++;
            cscRows[at] = i + base, cscVals[at] = cv[e];
        }
    for (int j = 0; j <= cols; ++j)
        cscPtr[j] += base;

    /* leg 2: A^T as HELL on the device, then to CSR: the CSC arrays of A */
    void* tWork = deviceAlloc(spgpuHellTransposeWorkBytes(rows, cols, slots));
    const int tHacks = (cols + hackSize - 1) / hackSize;
    int* tRs = (int*)deviceAlloc((size_t)cols * sizeof(int));
    int* tHackOffsets = (int*)deviceAlloc((size_t)tHacks * sizeof(int));
    int tLongest = 0, tNnz = 0, tHeight = 0;
    OK(spgpuHellTransposeLengthsDevice(h, tRs, &tLongest, &tNnz, rP, hackSize, hackOffsets, rS, NULL, rows, cols, base, slots, tWork));
    OK(spgpuHellPlanDevice(h, &tHeight, tHackOffsets, hackSize, cols, tRs, tWork));
    const int tSlots = hackSize * tHeight;
    double* tM = (double*)deviceAlloc((size_t)tSlots * sizeof(double));
    int* tP = (int*)deviceAlloc((size_t)tSlots * sizeof(int));
    CHECK(hipMemset(tM, 0, (size_t)tSlots * sizeof(double)));
    CHECK(hipMemset(tP, 0, (size_t)tSlots * sizeof(int)));
    OK(spgpuHellTransposeDevice(h, tM, tP, tHackOffsets, hackSize, base, cM, rP, hackSize, hackOffsets, rS, NULL, rows, cols, base, slots,
                                SPGPU_TYPE_DOUBLE, tRs, tWork));
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    const int leg2 = tNnz == nnz && hellToCsrEquals(h, tM, tP, hackSize, tHackOffsets, tRs, cols, tSlots, base, cscPtr, cscRows, cscVals, nnz);
    printf("HELL of A^T -> CSR against the CSC of A: %s\n", leg2 ? "OK" : "MISMATCH");

    spgpuDestroy(h);
    CHECK(hipGetLastError());
    return leg1 && leg2 ? 0 : 1;
}
