/*
 * The second level of an aggregation multigrid built with no array leaving the device, written against the C ABI only
 * (spgpu/ext/aggregate_device.h).  A is the 5-point Laplacian on an n x n grid (4 on the diagonal, -1 to each neighbour inside the
 * grid), listed as COO contributions with the diagonal split in two and assembled (spgpu/ext/assemble_device.h).  Base 1 everywhere.
 *   1. strength of connection at theta = 0.25 (spgpuCsrStrengthDevice): 1 >= (1/16 * 4) * 4, every neighbour is strong;
 *   2. the aggregates (spgpuCsrAggregateDevice) and the tentative prolongator T with unit entries (spgpuCsrTentativeDevice);
 *   3. T goes into HELL (spgpu/ext/csr_device.h), T^T comes out of spgpuHellTransposeDevice and back to CSR through
 *      spgpuHellToCsrDevice; R = T^T * A and A_c = R * T are formed by spgpuCsrSpgemmProductsDevice / PlanDevice / Device.
 * Every number is a small integer, so the checks -- made on copies fetched afterwards -- are ==: aggregateOf against a plain-C
 * restatement of the rounds (below), the sizes sum to n^2, A_c has one row per aggregate, the entries of A_c sum to the entries of A
 * (T has one unit entry per row, so 1^T A_c 1 = 1^T A 1), and the pattern of A_c is symmetric.
 *
 *   usage: amg_setup_amd [n=64]
 * Prints one summary line and exits non-zero on a mismatch.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/convert_device.h"
#include "spgpu/hell.h"
#include "spgpu/ext/aggregate_device.h"
#include "spgpu/ext/assemble_device.h"
#include "spgpu/ext/csr_device.h"
#include "spgpu/ext/spgemm_device.h"
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

enum { HACK = 32, BASE = 1 };

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

static void* hostCopyOf(const void* device, size_t bytes)
{
    void* p = malloc(bytes ? bytes : 16);
    CHECK(hipMemcpy(p, device, bytes, hipMemcpyDeviceToHost));
    return p;
}

typedef struct Csr {
    int rows, cols, nnz;
    int* ptr;
    int* idx;
    double* val;
} Csr;

typedef struct Hell {
    double* cM;
    int* rP;
    int* hackOffsets;
    int* rS;
    int slots, longest;
} Hell;

/* the HELL arrays of a CSR matrix */
static void hellOf(spgpuHandle_t h, Hell* m, const Csr* a, void* planWork)
{
    int height = 0;
    m->rS = (int*)deviceAlloc((size_t)a->rows * sizeof(int));
    OK(spgpuCsrRowLengthsDevice(h, m->rS, &m->longest, a->rows, a->ptr, BASE));
    m->hackOffsets = (int*)deviceAlloc((size_t)((a->rows + HACK - 1) / HACK) * sizeof(int));
    OK(spgpuHellPlanDevice(h, &height, m->hackOffsets, HACK, a->rows, m->rS, planWork));
    m->slots = HACK * height;
    m->cM = (double*)deviceAlloc((size_t)m->slots * sizeof(double));
    m->rP = (int*)deviceAlloc((size_t)m->slots * sizeof(int));
    CHECK(hipMemset(m->cM, 0, (size_t)m->slots * sizeof(double)));
    CHECK(hipMemset(m->rP, 0, (size_t)m->slots * sizeof(int)));
    OK(spgpuCsrToHellDevice(h, m->cM, m->rP, m->hackOffsets, HACK, BASE, a->rows, a->ptr, a->idx, a->val, BASE, SPGPU_TYPE_DOUBLE, NULL));
}

/* C = A * B: the analysis and the fill; the scratch is freed when the fill has passed on the stream */
static void multiply(spgpuHandle_t h, Csr* c, const Csr* a, const Csr* b)
{
    int products = 0;
    void* small = deviceAlloc(spgpuCsrSpgemmWorkBytes(a->rows, b->cols, 0));
    OK(spgpuCsrSpgemmProductsDevice(h, &products, a->rows, a->cols, a->ptr, a->idx, b->ptr, BASE, small));
    CHECK(hipFree(small));
    void* work = deviceAlloc(spgpuCsrSpgemmWorkBytes(a->rows, b->cols, products));
    c->rows = a->rows, c->cols = b->cols;
    c->ptr = (int*)deviceAlloc(((size_t)a->rows + 1) * sizeof(int));
    OK(spgpuCsrSpgemmPlanDevice(h, &c->nnz, c->ptr, a->rows, a->cols, b->cols, a->ptr, a->idx, b->ptr, b->idx, BASE, products, work));
    c->idx = (int*)deviceAlloc((size_t)c->nnz * sizeof(int));
    c->val = (double*)deviceAlloc((size_t)c->nnz * sizeof(double));
    OK(spgpuCsrSpgemmDevice(h, c->idx, c->val, c->nnz, a->rows, a->ptr, a->idx, a->val, b->ptr, b->idx, b->val, c->ptr, BASE, SPGPU_TYPE_DOUBLE,
                            work));
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    CHECK(hipFree(work));
}

/* ---- the contract of spgpu/ext/aggregate_device.h in plain C, on host copies of A ---- */
static unsigned priorityOf(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x >> 1;
}

typedef unsigned long long Tuple;

/* out[i] = max(in[i], max over the strong neighbours j of i of in[j]) */
static void sweepOnHost(Tuple* out, const Tuple* in, int rows, const int* ptr, const int* idx, const unsigned char* strong)
{
    for (int i = 0; i < rows; ++i) {
        Tuple best = in[i];
        for (int p = ptr[i] - BASE; p < ptr[i + 1] - BASE; ++p)
            if (strong[p] && idx[p] - BASE != i && in[idx[p] - BASE] > best)
                best = in[idx[p] - BASE];
        out[i] = best;
    }
}

/* one joining pass: an unassigned node takes the smallest aggregate number among its assigned strong neighbours in `in` */
static void joinOnHost(int* out, const int* in, int rows, const int* ptr, const int* idx, const unsigned char* strong)
{
    for (int i = 0; i < rows; ++i) {
        int mine = in[i];
        if (mine < 0)
            for (int p = ptr[i] - BASE; p < ptr[i + 1] - BASE; ++p) {
                const int j = idx[p] - BASE;
                if (strong[p] && j != i && in[j] >= 0 && (mine < 0 || in[j] < mine))
                    mine = in[j];
            }
        out[i] = mine;
    }
}

static void aggregateOnHost(int* aggregateOf, int* count, int* roundsOut, int rows, const int* ptr, const int* idx, const double* val, double theta)
{
    const int nnz = ptr[rows] - BASE;
    double* d = (double*)calloc((size_t)rows, sizeof(double));
    unsigned char* strong = (unsigned char*)calloc((size_t)(nnz ? nnz : 1), 1);
    for (int i = 0; i < rows; ++i)
        for (int p = ptr[i] - BASE; p < ptr[i + 1] - BASE; ++p)
            if (idx[p] - BASE == i) {
                d[i] = val[p] < 0 ? -val[p] : val[p];
                break;
            }
    const double t = theta * theta;
    for (int i = 0; i < rows; ++i)
        for (int p = ptr[i] - BASE; p < ptr[i + 1] - BASE; ++p) {
            const int j = idx[p] - BASE;
            const double lhs = val[p] * val[p], scaled = t * d[i];
            strong[p] = j != i && lhs >= scaled * d[j];
        }
    Tuple* t0 = (Tuple*)malloc((size_t)rows * sizeof(Tuple));
    Tuple* t1 = (Tuple*)malloc((size_t)rows * sizeof(Tuple));
    Tuple* t2 = (Tuple*)malloc((size_t)rows * sizeof(Tuple));
    const Tuple one = (Tuple)1 << 62;
    for (int i = 0; i < rows; ++i)
        t0[i] = one | ((Tuple)priorityOf((unsigned)i) << 31) | (Tuple)i; /* UNDECIDED */
    int rounds = 0, left = rows;
    while (left > 0) {
        sweepOnHost(t1, t0, rows, ptr, idx, strong);
        sweepOnHost(t2, t1, rows, ptr, idx, strong);
        left = 0;
        for (int i = 0; i < rows; ++i) {
            if ((t0[i] >> 62) != 1)
                continue;
            if (t2[i] == t0[i])
                t0[i] += one; /* ROOT */
            else if ((t2[i] >> 62) == 2)
                t0[i] -= one; /* OUT */
            else
                ++left;
        }
        ++rounds;
    }
    int* a0 = (int*)malloc((size_t)rows * sizeof(int));
    int* a1 = (int*)malloc((size_t)rows * sizeof(int));
    int roots = 0;
    for (int i = 0; i < rows; ++i)
        a0[i] = (t0[i] >> 62) == 2 ? roots++ : -1;
    joinOnHost(a1, a0, rows, ptr, idx, strong);
    joinOnHost(aggregateOf, a1, rows, ptr, idx, strong);
    *count = roots, *roundsOut = rounds;
    free(d), free(strong), free(t0), free(t1), free(t2), free(a0), free(a1);
}

/* is (row, column), both 0-based, stored?  Rows ascend. */
static int stored(const int* ptr, const int* idx, int row, int column)
{
    int lo = ptr[row] - BASE, hi = ptr[row + 1] - BASE;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (idx[mid] - BASE < column)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < ptr[row + 1] - BASE && idx[lo] - BASE == column;
}

int main(int argc, char** argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 64;
    if (n < 2 || n > 4000) {
        fprintf(stderr, "usage: amg_setup_amd [n: 2 .. 4000]\n");
        return 2;
    }
    const int fine = n * n;
    const double theta = 0.25;

    /* ---- A as a list of contributions: the diagonal as 3 + 1, each neighbour once ---- */
    int* ai = (int*)malloc((size_t)6 * fine * sizeof(int));
    int* aj = (int*)malloc((size_t)6 * fine * sizeof(int));
    double* av = (double*)malloc((size_t)6 * fine * sizeof(double));
    int listed = 0;
    for (int i = 0; i < fine; ++i) {
        const int x = i % n, y = i / n;
        const int to[4] = {x > 0 ? i - 1 : -1, x < n - 1 ? i + 1 : -1, y > 0 ? i - n : -1, y < n - 1 ? i + n : -1};
        for (int k = 0; k < 4; ++k)
            if (to[k] >= 0)
                ai[listed] = i + BASE, aj[listed] = to[k] + BASE, av[listed] = -1.0, ++listed;
        ai[listed] = i + BASE, aj[listed] = i + BASE, av[listed] = 3.0, ++listed;
        ai[listed] = i + BASE, aj[listed] = i + BASE, av[listed] = 1.0, ++listed;
    }

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS)
        return 2;
    int* dAi = (int*)deviceCopyOf(ai, (size_t)listed * sizeof(int));
    int* dAj = (int*)deviceCopyOf(aj, (size_t)listed * sizeof(int));
    double* dAv = (double*)deviceCopyOf(av, (size_t)listed * sizeof(double));
    void* planWork = deviceAlloc(spgpuCooConvertWorkBytes(fine, 0));

    /* ---- A assembled ---- */
    Csr A = {fine, fine, 0, NULL, NULL, NULL};
    A.ptr = (int*)deviceAlloc(((size_t)fine + 1) * sizeof(int));
    int* perm = (int*)deviceAlloc((size_t)listed * sizeof(int));
    int* segPtr = (int*)deviceAlloc(((size_t)listed + 1) * sizeof(int));
    void* asmWork = deviceAlloc(spgpuCooAssembleWorkBytes(fine, fine, listed));
    OK(spgpuCooAssemblePlanDevice(h, &A.nnz, A.ptr, perm, segPtr, fine, fine, listed, dAi, dAj, BASE, BASE, asmWork));
    CHECK(hipFree(asmWork));
    A.idx = (int*)deviceAlloc((size_t)A.nnz * sizeof(int));
    A.val = (double*)deviceAlloc((size_t)A.nnz * sizeof(double));
    OK(spgpuCooAssembleDevice(h, A.idx, A.val, A.nnz, listed, dAj, dAv, BASE, BASE, SPGPU_TYPE_DOUBLE, perm, segPtr));

    /* ---- strength, aggregates, T ---- */
    unsigned char* strong = (unsigned char*)deviceAlloc((size_t)A.nnz);
    double* diagAbs = (double*)deviceAlloc((size_t)fine * sizeof(double));
    OK(spgpuCsrStrengthDevice(h, strong, diagAbs, fine, A.ptr, A.idx, A.val, BASE, theta, SPGPU_TYPE_DOUBLE));
    int aggregates = 0, rounds = 0;
    int* aggregateOf = (int*)deviceAlloc((size_t)fine * sizeof(int));
    int* aggregateSize = (int*)deviceAlloc((size_t)fine * sizeof(int));
    void* aggWork = deviceAlloc(spgpuCsrAggregateWorkBytes(fine));
    OK(spgpuCsrAggregateDevice(h, &aggregates, &rounds, aggregateOf, aggregateSize, fine, A.ptr, A.idx, strong, BASE, aggWork));
    CHECK(hipFree(aggWork));
    const int coarse = aggregates;
    Csr T = {fine, coarse, fine, NULL, NULL, NULL};
    T.ptr = (int*)deviceAlloc(((size_t)fine + 1) * sizeof(int));
    T.idx = (int*)deviceAlloc((size_t)fine * sizeof(int));
    T.val = (double*)deviceAlloc((size_t)fine * sizeof(double));
    OK(spgpuCsrTentativeDevice(h, T.ptr, T.idx, T.val, fine, aggregateOf, NULL, BASE, SPGPU_TYPE_DOUBLE));

    /* ---- T^T through the transpose and back to CSR ---- */
    Hell hp, ht;
    hellOf(h, &hp, &T, planWork);
    void* tWork = deviceAlloc(spgpuHellTransposeWorkBytes(fine, coarse, hp.slots));
    int tNnz = 0, tHeight = 0;
    ht.rS = (int*)deviceAlloc((size_t)coarse * sizeof(int));
    OK(spgpuHellTransposeLengthsDevice(h, ht.rS, &ht.longest, &tNnz, hp.rP, HACK, hp.hackOffsets, hp.rS, NULL, fine, coarse, BASE, hp.slots, tWork));
    ht.hackOffsets = (int*)deviceAlloc((size_t)((coarse + HACK - 1) / HACK) * sizeof(int));
    OK(spgpuHellPlanDevice(h, &tHeight, ht.hackOffsets, HACK, coarse, ht.rS, tWork));
    ht.slots = HACK * tHeight;
    ht.cM = (double*)deviceAlloc((size_t)ht.slots * sizeof(double));
    ht.rP = (int*)deviceAlloc((size_t)ht.slots * sizeof(int));
    CHECK(hipMemset(ht.cM, 0, (size_t)ht.slots * sizeof(double)));
    CHECK(hipMemset(ht.rP, 0, (size_t)ht.slots * sizeof(int)));
    OK(spgpuHellTransposeDevice(h, ht.cM, ht.rP, ht.hackOffsets, HACK, BASE, hp.cM, hp.rP, HACK, hp.hackOffsets, hp.rS, NULL, fine, coarse, BASE,
                                hp.slots, SPGPU_TYPE_DOUBLE, ht.rS, tWork));
    Csr TT = {coarse, fine, 0, NULL, NULL, NULL};
    int ttLongest = 0;
    void* csrWork = deviceAlloc(spgpuToCsrWorkBytes(coarse));
    TT.ptr = (int*)deviceAlloc(((size_t)coarse + 1) * sizeof(int));
    OK(spgpuHellToCsrRowPtrDevice(h, TT.ptr, &TT.nnz, &ttLongest, BASE, HACK, ht.hackOffsets, ht.rS, NULL, coarse, ht.slots, csrWork));
    TT.idx = (int*)deviceAlloc((size_t)TT.nnz * sizeof(int));
    TT.val = (double*)deviceAlloc((size_t)TT.nnz * sizeof(double));
    OK(spgpuHellToCsrDevice(h, TT.idx, TT.val, TT.ptr, BASE, ht.cM, ht.rP, HACK, ht.hackOffsets, ht.rS, NULL, coarse, BASE, SPGPU_TYPE_DOUBLE));

    /* ---- R = T^T * A, A_c = R * T ---- */
    Csr R, Ac;
    multiply(h, &R, &TT, &A);
    multiply(h, &Ac, &R, &T);
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));

    /* ---- the checks, on copies ---- */
    int* aPtr = (int*)hostCopyOf(A.ptr, ((size_t)fine + 1) * sizeof(int));
    int* aIdx = (int*)hostCopyOf(A.idx, (size_t)A.nnz * sizeof(int));
    double* aVal = (double*)hostCopyOf(A.val, (size_t)A.nnz * sizeof(double));
    unsigned char* strongHost = (unsigned char*)hostCopyOf(strong, (size_t)A.nnz);
    int* ofHost = (int*)hostCopyOf(aggregateOf, (size_t)fine * sizeof(int));
    int* sizeHost = (int*)hostCopyOf(aggregateSize, (size_t)coarse * sizeof(int));
    int* cPtr = (int*)hostCopyOf(Ac.ptr, ((size_t)coarse + 1) * sizeof(int));
    int* cIdx = (int*)hostCopyOf(Ac.idx, (size_t)Ac.nnz * sizeof(int));
    double* cVal = (double*)hostCopyOf(Ac.val, (size_t)Ac.nnz * sizeof(double));
    int failed = 0, wantCount = 0, wantRounds = 0, strongCount = 0, sizesSum = 0, symmetric = 1;
    int* wantOf = (int*)malloc((size_t)fine * sizeof(int));
    aggregateOnHost(wantOf, &wantCount, &wantRounds, fine, aPtr, aIdx, aVal, theta);
    if (wantCount != aggregates || wantRounds != rounds) {
        printf("the device found %d aggregates in %d rounds, the restatement %d in %d\n", aggregates, rounds, wantCount, wantRounds);
        failed = 1;
    }
    for (int i = 0; i < fine && !failed; ++i)
        if (ofHost[i] != wantOf[i]) {
            printf("aggregateOf[%d] = %d, the restatement gives %d\n", i, ofHost[i], wantOf[i]);
            failed = 1;
        }
    for (int p = 0; p < A.nnz; ++p)
        strongCount += strongHost[p];
    for (int a = 0; a < coarse; ++a)
        sizesSum += sizeHost[a];
    if (sizesSum != fine) {
        printf("the sizes sum to %d, not to %d\n", sizesSum, fine);
        failed = 1;
    }
    if (Ac.rows != aggregates || Ac.cols != aggregates || TT.nnz != fine || cPtr[coarse] - BASE != Ac.nnz) {
        printf("A_c is %d x %d with %d entries for %d aggregates; T^T has %d entries\n", Ac.rows, Ac.cols, Ac.nnz, aggregates, TT.nnz);
        failed = 1;
    }
    double sumA = 0.0, sumAc = 0.0;
    for (int p = 0; p < A.nnz; ++p)
        sumA += aVal[p];
    for (int p = 0; p < Ac.nnz; ++p)
        sumAc += cVal[p];
    if (sumA != sumAc) {
        printf("the entries of A_c sum to %.17g, those of A to %.17g\n", sumAc, sumA);
        failed = 1;
    }
    for (int I = 0; I < coarse && symmetric; ++I)
        for (int p = cPtr[I] - BASE; p < cPtr[I + 1] - BASE; ++p)
            if (!stored(cPtr, cIdx, cIdx[p] - BASE, I)) {
                printf("A_c stores (%d, %d) but not (%d, %d)\n", I, cIdx[p] - BASE, cIdx[p] - BASE, I);
                symmetric = 0;
                break;
            }
    failed |= !symmetric;
    printf("amg_setup n=%d rows=%d entries=%d strong=%d aggregates=%d rounds=%d sizes_sum=%d coarse_rows=%d coarse_entries=%d sum_a=%.17g "
           "sum_ac=%.17g symmetric=%d %s\n",
           n, fine, A.nnz, strongCount, aggregates, rounds, sizesSum, Ac.rows, Ac.nnz, sumA, sumAc, symmetric, failed ? "FAILED" : "PASSED");
    spgpuDestroy(h);
    CHECK(hipGetLastError());
    return failed;
}
