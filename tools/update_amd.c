/*
 * New coefficients for a stored HELL matrix (spgpu/ext/update_device.h), written against the C ABI only: what a solver that
 * re-assembles its matrix at every step does.  A small ragged CSR matrix (row i of (i * 7) % 23 entries, columns ascending, base
 * 1) goes into HELL in HBM with spgpuCsrToHellDevice and is multiplied; then all its coefficients are replaced with
 * spgpuCsrToHellValuesDevice and it is multiplied again; then every third entry is overwritten through spgpuDhellcsput (a
 * list in reverse order, with a row below the base and a column that is not stored among its entries) and it is multiplied a
 * third time.  The whole runs twice: rows as they come, and stored in reverse row order (rIdx; rowOf from
 * spgpuInvertRowOrderDevice) -- the same matrix, so the same numbers.
 *
 * Every coefficient and every x[j] is a small multiple of 1/8: all sums are exact in fp64 in any order, and the checksums
 * printed here can be compared with == against a computation anywhere else (tests/test_gpu_update_tool.py: numpy).
 *
 *   usage: update_amd [rows=1000]
 * Prints "<order> <stage>: sum(z) sum((i % 7 + 1) * z[i]) sum(cM)" for the three stages of both orders.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/convert_device.h"
#include "spgpu/hell.h"
#include "spgpu/ext/csr_device.h"
#include "spgpu/ext/update_device.h"

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

/* multiply, bring z and cM back, print the three sums of the stage */
static void report(spgpuHandle_t h, const char* order, const char* stage, double* z, const double* cM, const int* rP, int hackSize,
                   const int* hackOffsets, const int* rS, const int* rIdx, int rows, const double* x, int base, int slots)
{
    spgpuDhellspmv(h, z, z, 1.0, cM, rP, hackSize, hackOffsets, rS, rIdx, 0, rows, x, 0.0, base);
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    double* hz = (double*)malloc((size_t)rows * sizeof(double));
    double* hm = (double*)malloc((size_t)(slots ? slots : 1) * sizeof(double));
    CHECK(hipMemcpy(hz, z, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hm, cM, (size_t)slots * sizeof(double), hipMemcpyDeviceToHost));
    double plain = 0.0, weighted = 0.0, stored = 0.0;
    for (int i = 0; i < rows; ++i)
        plain += hz[i], weighted += (double)(i % 7 + 1) * hz[i];
    for (int s = 0; s < slots; ++s)
        stored += hm[s];
    printf("%s %s: %.17g %.17g %.17g\n", order, stage, plain, weighted, stored);
    free(hz);
    free(hm);
}

int main(int argc, char** argv)
{
    const int rows = argc > 1 ? atoi(argv[1]) : 1000;
    const int hackSize = 32, base = 1;
    if (rows < 1 || rows > 1000000) {
        fprintf(stderr, "usage: update_amd [rows]\n");
        return 2;
    }
    const int cols = rows + 80;

    /* the caller's CSR, base 1: row i holds columns i % 11 + 3 k (ascending), first values e / 4 + 1 / 4 */
    int* ptr = (int*)malloc(((size_t)rows + 1) * sizeof(int));
    ptr[0] = base;
    for (int i = 0; i < rows; ++i)
        ptr[i + 1] = ptr[i] + (int)(((long long)i * 7) % 23);
    const int nnz = ptr[rows] - base;
    int* ci = (int*)malloc((size_t)(nnz ? nnz : 1) * sizeof(int));
    double* v1 = (double*)malloc((size_t)(nnz ? nnz : 1) * sizeof(double));
    double* v2 = (double*)malloc((size_t)(nnz ? nnz : 1) * sizeof(double));
    for (int i = 0; i < rows; ++i)
        for (int e = ptr[i] - base, k = 0; e < ptr[i + 1] - base; ++e, ++k) {
            ci[e] = i % 11 + 3 * k + base;
            v1[e] = (double)e * 0.25 + 0.25;
            v2[e] = -(double)(e % 1001) * 0.5 - 0.75;
        }
    double* x = (double*)malloc((size_t)cols * sizeof(double));
    for (int j = 0; j < cols; ++j)
        x[j] = (double)(j % 13) * 0.5 + 1.0;

    /* the csput list, back to front: every third entry of every row gets (i % 97) * 2 + 1 / 8; in front of it an entry whose
     * row lies below the base and one whose column (a multiple of 3 away from no stored one) is not in its row */
    int listed = 2;
    for (int i = 0; i < rows; ++i)
        listed += (ptr[i + 1] - ptr[i] + 2) / 3;
    int* aI = (int*)malloc((size_t)listed * sizeof(int));
    int* aJ = (int*)malloc((size_t)listed * sizeof(int));
    double* aV = (double*)malloc((size_t)listed * sizeof(double));
    int at = listed;
    for (int i = 0; i < rows; ++i)
        for (int e = ptr[i] - base; e < ptr[i + 1] - base; e += 3) {
            --at;
            aI[at] = i + base, aJ[at] = ci[e], aV[at] = (double)(i % 97) * 2.0 + 0.125;
        }
    aI[1] = base - 1, aJ[1] = base, aV[1] = 1000.0;                  /* row -1 */
    aI[0] = rows / 2 + base, aJ[0] = (rows / 2) % 11 + 1 + base, aV[0] = 2000.0; /* a column between two stored ones, or in an empty row */
    if (at != 2)
        return 2;

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS)
        return 2;
    int* dPtr = (int*)deviceCopyOf(ptr, ((size_t)rows + 1) * sizeof(int));
    int* dCi = (int*)deviceCopyOf(ci, (size_t)nnz * sizeof(int));
    double* dV1 = (double*)deviceCopyOf(v1, (size_t)nnz * sizeof(double));
    double* dV2 = (double*)deviceCopyOf(v2, (size_t)nnz * sizeof(double));
    double* dX = (double*)deviceCopyOf(x, (size_t)cols * sizeof(double));
    int* dAi = (int*)deviceCopyOf(aI, (size_t)listed * sizeof(int));
    int* dAj = (int*)deviceCopyOf(aJ, (size_t)listed * sizeof(int));
    double* dAv = (double*)deviceCopyOf(aV, (size_t)listed * sizeof(double));
    double* z = (double*)deviceAlloc((size_t)rows * sizeof(double));
    const int hacks = (rows + hackSize - 1) / hackSize;
    void* planWork = deviceAlloc(spgpuCooConvertWorkBytes(rows, 0));
    printf("A: %d x %d, %d entries, %d list entries (hackSize %d)\n", rows, cols, nnz, listed, hackSize);

    for (int ordered = 0; ordered < 2; ++ordered) {
        const char* order = ordered ? "reversed" : "natural";
        /* storage row r holds matrix row rIdx[r] = rows - 1 - r; its lengths in storage order */
        int* hostOrder = (int*)malloc((size_t)rows * sizeof(int));
        int* hostLengths = (int*)malloc((size_t)rows * sizeof(int));
        for (int r = 0; r < rows; ++r) {
            hostOrder[r] = ordered ? rows - 1 - r : r;
            hostLengths[r] = ptr[hostOrder[r] + 1] - ptr[hostOrder[r]];
        }
        int* rIdx = ordered ? (int*)deviceCopyOf(hostOrder, (size_t)rows * sizeof(int)) : NULL;
        int* rS = (int*)deviceCopyOf(hostLengths, (size_t)rows * sizeof(int));
        int* rowOf = NULL;
        if (ordered) {
            rowOf = (int*)deviceAlloc((size_t)rows * sizeof(int));
            CHECK(hipMemset(rowOf, 0xFF, (size_t)rows * sizeof(int)));
            OK(spgpuInvertRowOrderDevice(h, rowOf, rIdx, rows));
        }
        int* hackOffsets = (int*)deviceAlloc((size_t)hacks * sizeof(int));
        int height = 0;
        OK(spgpuHellPlanDevice(h, &height, hackOffsets, hackSize, rows, rS, planWork));
        const int slots = hackSize * height;
        double* cM = (double*)deviceAlloc((size_t)slots * sizeof(double));
        int* rP = (int*)deviceAlloc((size_t)slots * sizeof(int));
        CHECK(hipMemset(cM, 0, (size_t)slots * sizeof(double)));
        CHECK(hipMemset(rP, 0, (size_t)slots * sizeof(int)));

        OK(spgpuCsrToHellDevice(h, cM, rP, hackOffsets, hackSize, base, rows, dPtr, dCi, dV1, base, SPGPU_TYPE_DOUBLE, rIdx));
        report(h, order, "built", z, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, dX, base, slots);
        OK(spgpuCsrToHellValuesDevice(h, cM, hackOffsets, hackSize, rows, dPtr, dV2, base, SPGPU_TYPE_DOUBLE, rIdx));
        report(h, order, "refilled", z, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, dX, base, slots);
        spgpuDhellcsput(h, 1.0, cM, rP, hackSize, hackOffsets, rS, rowOf, rows, listed, dAi, dAj, dAv, base);
        report(h, order, "csput", z, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, dX, base, slots);

        CHECK(hipFree(cM));
        CHECK(hipFree(rP));
        CHECK(hipFree(hackOffsets));
        CHECK(hipFree(rS));
        if (ordered) {
            CHECK(hipFree(rIdx));
            CHECK(hipFree(rowOf));
        }
        free(hostOrder);
        free(hostLengths);
    }
    spgpuDestroy(h);
    CHECK(hipGetLastError());
    return 0;
}
