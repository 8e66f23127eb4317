/*
 * A multicolour order through spgpu/ext/colour_device.h, written against the C ABI only.  A is the 7-point Laplacian on a g^3 grid
 * with the diagonal 6 + (i % 3) / 4 (symmetric, diagonally dominant), held WHOLE in CSR in its natural order.
 *
 *   (a) A is coloured, the rows are listed colour by colour and B = A(order, order) is formed, all on the device; order, inverse
 *       and B are compared with a restatement in plain C: order is sorted by (colour, row), inverse is its inverse, and B equals
 *       P A P^T entry for entry, rows ascending (bit for bit: the values are moved);
 *   (b) the lower and upper Plans of spgpu/ext/trsv_device.h on A and on B: the level counts of both orders;
 *   (c) CG preconditioned by symmetric Gauss-Seidel, as tools/gs_amd.c runs it, once on A with b and once on B with the gathered
 *       b (spgpuDgath by order); the solution of B is mapped back (spgpuDgath by inverse).  Iterations and time of both: a
 *       multicolour order has far fewer levels, so an iteration is cheaper, and it usually needs more iterations.
 *
 *   usage: multicolour_amd [grid=8] [maxIter=2000] [tol=1e-8]
 * Exits 0 iff (a) matches, B has no more levels than colours on either side, and both solves converged: the recursion's relative
 * residual meets tol, the bound of gs_amd, and the residual ||b - A x|| / ||b|| recomputed on the host in A's own order, which
 * rounding separates from the recursion's, stays within 10 tol for both solutions.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "spgpu/core.h"
#include "spgpu/ell_conv.h"
#include "spgpu/hell.h"
#include "spgpu/hell_conv.h"
#include "spgpu/vector.h"
#include "spgpu/ext/colour_device.h"
#include "spgpu/ext/trsv_device.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)
#define OK(call)                                                                  \
    do {                                                                          \
        if ((call) != SPGPU_SUCCESS) {                                            \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #call);     \
            exit(2);                                                              \
        }                                                                         \
    } while (0)

enum { HACK = 32 };

typedef struct {
    int levels;
    int *order, *levelPtr, *levelPtrHost;
} Plan;

/* one matrix on the device: CSR for the two solves, HELL for the product, the diagonal for the middle of the preconditioner */
typedef struct {
    int n, nnz, maxRow;
    int *dPtr, *dIdx, *dHi, *dHo, *dRs;
    double *dVal, *dHv, *dDiag;
    Plan lower, upper;
} Matrix;

static Plan makePlan(spgpuHandle_t h, int n, const int* dPtr, const int* dIdx, int side)
{
    Plan p;
    void* work;
    CHECK(hipMalloc((void**)&p.order, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&p.levelPtr, ((size_t)n + 1) * sizeof(int)));
    p.levelPtrHost = (int*)malloc(((size_t)n + 1) * sizeof(int));
    CHECK(hipMalloc(&work, spgpuCsrTrsvWorkBytes(n)));
    OK(spgpuCsrTrsvPlanDevice(h, &p.levels, p.order, p.levelPtr, p.levelPtrHost, n, dPtr, dIdx, 0, side, SPGPU_TRSV_DIAG_STORED, work));
    CHECK(hipFree(work));
    return p;
}

/* the HELL arrays and the diagonal from host CSR (base 0); the CSR arrays themselves are on the device already */
static void finishMatrix(spgpuHandle_t h, Matrix* m, const int* ptr, const int* idx, const double* val)
{
    const int n = m->n, nnz = m->nnz;
    int* cr = (int*)malloc((size_t)nnz * sizeof(int));
    double* diagonal = (double*)calloc(n, sizeof(double));
    for (int i = 0; i < n; ++i)
        for (int e = ptr[i]; e < ptr[i + 1]; ++e) {
            cr[e] = i;
            if (idx[e] == i)
                diagonal[i] = val[e];
        }
    int maxRow = 0, height = 0;
    int* rowLen = (int*)malloc((size_t)n * sizeof(int));
    computeEllRowLenghts(rowLen, &maxRow, n, nnz, cr, 0);
    const int pitch = computeEllAllocPitch(n);
    double* ev = (double*)calloc((size_t)maxRow * pitch, sizeof(double));
    int* ei = (int*)calloc((size_t)maxRow * pitch, sizeof(int));
    cooToEll(ev, ei, pitch, pitch, maxRow, 0, n, nnz, cr, idx, val, 0, SPGPU_TYPE_DOUBLE);
    computeHellAllocSize(&height, HACK, n, rowLen);
    const int hacks = (n + HACK - 1) / HACK;
    double* hv = (double*)calloc((size_t)HACK * height, sizeof(double));
    int* hi = (int*)calloc((size_t)HACK * height, sizeof(int));
    int* ho = (int*)calloc(hacks, sizeof(int));
    ellToHell(hv, hi, ho, HACK, ev, ei, pitch, pitch, rowLen, n, SPGPU_TYPE_DOUBLE);
    m->maxRow = maxRow;
    CHECK(hipMalloc((void**)&m->dHv, (size_t)HACK * height * sizeof(double)));
    CHECK(hipMalloc((void**)&m->dHi, (size_t)HACK * height * sizeof(int)));
    CHECK(hipMalloc((void**)&m->dHo, hacks * sizeof(int)));
    CHECK(hipMalloc((void**)&m->dRs, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&m->dDiag, (size_t)n * sizeof(double)));
    CHECK(hipMemcpy(m->dHv, hv, (size_t)HACK * height * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(m->dHi, hi, (size_t)HACK * height * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(m->dHo, ho, hacks * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(m->dRs, rowLen, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(m->dDiag, diagonal, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    m->lower = makePlan(h, n, m->dPtr, m->dIdx, SPGPU_TRSV_LOWER);
    m->upper = makePlan(h, n, m->dPtr, m->dIdx, SPGPU_TRSV_UPPER);
    free(cr); free(diagonal); free(rowLen); free(ev); free(ei); free(hv); free(hi); free(ho);
}

static double seconds(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

typedef struct {
    int iterations, converged;
    double relative, milliseconds;
} Solve;

/* CG on m, preconditioned by z = (D + U)^-1 D (D + L)^-1 r, from x = 0; dB is left as it was */
static Solve sgsPcg(spgpuHandle_t h, const Matrix* m, double* dX, const double* dB, int maxIter, double tol)
{
    const int n = m->n;
    const size_t vecBytes = (size_t)n * sizeof(double);
    hipStream_t stream = spgpuGetStream(h);
    double *dR, *dP, *dAp, *dZ, *dT;
    CHECK(hipMalloc((void**)&dR, vecBytes));
    CHECK(hipMalloc((void**)&dP, vecBytes));
    CHECK(hipMalloc((void**)&dAp, vecBytes));
    CHECK(hipMalloc((void**)&dZ, vecBytes));
    CHECK(hipMalloc((void**)&dT, vecBytes));
#define SOLVE(plan, side, out, in)                                                                                                     \
    OK(spgpuCsrTrsvDevice(h, out, in, n, (plan).levels, (plan).order, (plan).levelPtr, (plan).levelPtrHost, m->dPtr, m->dIdx, m->dVal, 0, \
                          side, SPGPU_TRSV_DIAG_STORED, SPGPU_TYPE_DOUBLE))
#define PRECONDITION()                                   \
    do {                                                 \
        SOLVE(m->lower, SPGPU_TRSV_LOWER, dT, dR);       \
        spgpuDaxy(h, dT, n, 1.0, m->dDiag, dT);          \
        SOLVE(m->upper, SPGPU_TRSV_UPPER, dZ, dT);       \
    } while (0)
    CHECK(hipMemcpy(dR, dB, vecBytes, hipMemcpyDeviceToDevice));
    CHECK(hipMemset(dX, 0, vecBytes));
    CHECK(hipDeviceSynchronize());
    const double start = seconds();
    PRECONDITION();
    CHECK(hipMemcpyAsync(dP, dZ, vecBytes, hipMemcpyDeviceToDevice, stream));
    double rz = spgpuDdot(h, n, dR, dZ);
    double rr = spgpuDdot(h, n, dR, dR);
    const double rr0 = rr;
    int it = 0;
    while (it < maxIter && sqrt(rr / rr0) > tol) {
        spgpuDhellspmv(h, dAp, dAp, 1.0, m->dHv, m->dHi, HACK, m->dHo, m->dRs, NULL, m->maxRow, n, dP, 0.0, 0);
        const double alpha = rz / spgpuDdot(h, n, dP, dAp);
        spgpuDaxpby(h, dX, n, 1.0, dX, alpha, dP);
        spgpuDaxpby(h, dR, n, 1.0, dR, -alpha, dAp);
        PRECONDITION();
        const double rzNew = spgpuDdot(h, n, dR, dZ);
        rr = spgpuDdot(h, n, dR, dR);
        spgpuDaxpby(h, dP, n, rzNew / rz, dP, 1.0, dZ);
        rz = rzNew;
        ++it;
    }
    CHECK(hipStreamSynchronize(stream));
    Solve s;
    s.milliseconds = 1e3 * (seconds() - start);
    s.iterations = it;
    s.relative = sqrt(rr / rr0);
    s.converged = s.relative <= tol;
#undef PRECONDITION
#undef SOLVE
    CHECK(hipFree(dR)); CHECK(hipFree(dP)); CHECK(hipFree(dAp)); CHECK(hipFree(dZ)); CHECK(hipFree(dT));
    return s;
}

/* ||b - A x|| / ||b|| on the host, A in its natural order */
static double hostResidual(int n, const int* ptr, const int* idx, const double* val, const double* x, const double* b)
{
    double rr = 0, bb = 0;
    for (int i = 0; i < n; ++i) {
        double r = b[i];
        for (int e = ptr[i]; e < ptr[i + 1]; ++e)
            r -= val[e] * x[idx[e]];
        rr += r * r;
        bb += b[i] * b[i];
    }
    return sqrt(rr / bb);
}

int main(int argc, char** argv)
{
    const int g = argc > 1 ? atoi(argv[1]) : 8;
    const int maxIter = argc > 2 ? atoi(argv[2]) : 2000;
    const double tol = argc > 3 ? atof(argv[3]) : 1e-8;
    if (g < 2 || g > 1000 || maxIter < 1) {
        fprintf(stderr, "usage: multicolour_amd [grid=8] [maxIter=2000] [tol=1e-8]\n");
        return 2;
    }
    const int n = g * g * g;

    /* A in CSR (base 0, columns ascending) */
    int nnz = 0;
    int* ptr = (int*)malloc(((size_t)n + 1) * sizeof(int));
    int* idx = (int*)malloc((size_t)7 * n * sizeof(int));
    double* val = (double*)malloc((size_t)7 * n * sizeof(double));
#define ENTRY(j, v) { idx[nnz] = (j); val[nnz++] = (v); }
    for (int i = 0; i < n; ++i) {
        const int gx = i % g, gy = (i / g) % g, gz = i / (g * g);
        ptr[i] = nnz;
        if (gz > 0)     ENTRY(i - g * g, -1.0)
        if (gy > 0)     ENTRY(i - g, -1.0)
        if (gx > 0)     ENTRY(i - 1, -1.0)
        ENTRY(i, 6.0 + (i % 3) * 0.25)
        if (gx < g - 1) ENTRY(i + 1, -1.0)
        if (gy < g - 1) ENTRY(i + g, -1.0)
        if (gz < g - 1) ENTRY(i + g * g, -1.0)
    }
#undef ENTRY
    ptr[n] = nnz;
    /* b = A * xTrue, xTrue_i = 1 + (i % 7) / 8 */
    double* b = (double*)calloc(n, sizeof(double));
    for (int i = 0; i < n; ++i)
        for (int e = ptr[i]; e < ptr[i + 1]; ++e)
            b[i] += val[e] * (1.0 + (idx[e] % 7) * 0.125);

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS) return 2;
    hipStream_t stream = spgpuGetStream(h);
    const size_t vecBytes = (size_t)n * sizeof(double);
    Matrix A, B;
    A.n = B.n = n;
    A.nnz = B.nnz = nnz;
    CHECK(hipMalloc((void**)&A.dPtr, ((size_t)n + 1) * sizeof(int)));
    CHECK(hipMalloc((void**)&A.dIdx, (size_t)nnz * sizeof(int)));
    CHECK(hipMalloc((void**)&A.dVal, (size_t)nnz * sizeof(double)));
    CHECK(hipMalloc((void**)&B.dPtr, ((size_t)n + 1) * sizeof(int)));
    CHECK(hipMalloc((void**)&B.dIdx, (size_t)nnz * sizeof(int)));
    CHECK(hipMalloc((void**)&B.dVal, (size_t)nnz * sizeof(double)));
    CHECK(hipMemcpy(A.dPtr, ptr, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(A.dIdx, idx, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(A.dVal, val, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));

    /* ---- (a) colour, order, permute ---- */
    int colours = 0, rounds = 0;
    int *dColourOf, *dOrder, *dInverse, *dColourPtr;
    void *work, *permuteWork;
    CHECK(hipMalloc((void**)&dColourOf, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&dOrder, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&dInverse, (size_t)n * sizeof(int)));
    CHECK(hipMalloc(&work, spgpuCsrColourWorkBytes(n)));
    CHECK(hipMalloc(&permuteWork, spgpuCsrPermuteWorkBytes(n)));
    const double setupStart = seconds();
    OK(spgpuCsrColourDevice(h, &colours, &rounds, dColourOf, n, A.dPtr, A.dIdx, 0, work));
    CHECK(hipMalloc((void**)&dColourPtr, ((size_t)colours + 1) * sizeof(int)));
    OK(spgpuCsrColourOrderDevice(h, dOrder, dInverse, dColourPtr, n, colours, dColourOf, work));
    OK(spgpuCsrPermuteDevice(h, B.dPtr, B.dIdx, B.dVal, n, dOrder, dInverse, A.dPtr, A.dIdx, A.dVal, 0, SPGPU_TYPE_DOUBLE, permuteWork));
    CHECK(hipStreamSynchronize(stream));
    const double setupMs = 1e3 * (seconds() - setupStart);
    int* colourOf = (int*)malloc((size_t)n * sizeof(int));
    int* order = (int*)malloc((size_t)n * sizeof(int));
    int* inverse = (int*)malloc((size_t)n * sizeof(int));
    int* bPtr = (int*)malloc(((size_t)n + 1) * sizeof(int));
    int* bIdx = (int*)malloc((size_t)nnz * sizeof(int));
    double* bVal = (double*)malloc((size_t)nnz * sizeof(double));
    CHECK(hipMemcpy(colourOf, dColourOf, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(order, dOrder, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(inverse, dInverse, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(bPtr, B.dPtr, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(bIdx, B.dIdx, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(bVal, B.dVal, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
    /* the restatement: a proper colouring inside [0, colours), order sorted by (colour, row), inverse its inverse ... */
    int wrong = 0;
    for (int i = 0; i < n; ++i) {
        wrong += colourOf[i] < 0 || colourOf[i] >= colours;
        for (int e = ptr[i]; e < ptr[i + 1]; ++e)
            wrong += idx[e] != i && colourOf[idx[e]] == colourOf[i];
    }
    for (int k = 0; k < n; ++k) {
        wrong += order[k] < 0 || order[k] >= n || inverse[order[k] < 0 || order[k] >= n ? 0 : order[k]] != k;
        if (k > 0 && !wrong) {
            const int c0 = colourOf[order[k - 1]], c1 = colourOf[order[k]];
            wrong += c0 > c1 || (c0 == c1 && order[k - 1] >= order[k]);
        }
    }
    /* ... and B = P A P^T: row k of B is row order[k] of A with the columns renamed and sorted (an insertion sort: 7 entries) */
    int position = 0;
    for (int k = 0; k < n && !wrong; ++k) {
        const int row = order[k], length = ptr[row + 1] - ptr[row];
        int cols[7];
        double vals[7];
        for (int e = 0; e < length; ++e) {
            const int c = inverse[idx[ptr[row] + e]];
            const double v = val[ptr[row] + e];
            int at = e;
            while (at > 0 && cols[at - 1] > c) {
                cols[at] = cols[at - 1];
                vals[at] = vals[at - 1];
                --at;
            }
            cols[at] = c;
            vals[at] = v;
        }
        wrong += bPtr[k] != position;
        for (int e = 0; e < length && !wrong; ++e)
            wrong += bIdx[position + e] != cols[e] || memcmp(&bVal[position + e], &vals[e], sizeof(double)) != 0;
        position += length;
    }
    wrong += bPtr[n] != nnz;
    printf("multicolour order of the %d^3 7-point Laplacian (%d rows, %d nnz): %d colours in %d rounds, set-up %.3f ms, B %s P A P^T\n", g, n, nnz,
           colours, rounds, setupMs, wrong ? "DIFFERS from" : "equal to");

    /* ---- (b) the Plans ---- */
    finishMatrix(h, &A, ptr, idx, val);
    finishMatrix(h, &B, bPtr, bIdx, bVal);
    printf("levels below / above the diagonal: natural order %d / %d, multicolour order %d / %d\n", A.lower.levels, A.upper.levels, B.lower.levels,
           B.upper.levels);
    const int fewLevels = B.lower.levels <= colours && B.upper.levels <= colours;

    /* ---- (c) SGS-PCG on both orders ---- */
    double *dB, *dBp, *dX, *dXp, *dXBack;
    CHECK(hipMalloc((void**)&dB, vecBytes));
    CHECK(hipMalloc((void**)&dBp, vecBytes));
    CHECK(hipMalloc((void**)&dX, vecBytes));
    CHECK(hipMalloc((void**)&dXp, vecBytes));
    CHECK(hipMalloc((void**)&dXBack, vecBytes));
    CHECK(hipMemcpy(dB, b, vecBytes, hipMemcpyHostToDevice));
    spgpuDgath(h, dBp, n, dOrder, 0, dB); /* b on the new order */
    const Solve natural = sgsPcg(h, &A, dX, dB, maxIter, tol);
    const Solve coloured = sgsPcg(h, &B, dXp, dBp, maxIter, tol);
    spgpuDgath(h, dXBack, n, dInverse, 0, dXp); /* x back on the old order */
    CHECK(hipStreamSynchronize(stream));
    double* x = (double*)malloc(vecBytes);
    double* xBack = (double*)malloc(vecBytes);
    CHECK(hipMemcpy(x, dX, vecBytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(xBack, dXBack, vecBytes, hipMemcpyDeviceToHost));
    const double resNatural = hostResidual(n, ptr, idx, val, x, b), resColoured = hostResidual(n, ptr, idx, val, xBack, b);
    double apart = 0;
    for (int i = 0; i < n; ++i)
        apart = fabs(x[i] - xBack[i]) > apart ? fabs(x[i] - xBack[i]) : apart;
    printf("SGS-PCG natural order:     %d iterations, %.3f ms, relative residual %.3e (%s), on the host %.3e\n", natural.iterations,
           natural.milliseconds, natural.relative, natural.converged ? "converged" : "NOT converged", resNatural);
    printf("SGS-PCG multicolour order: %d iterations, %.3f ms, relative residual %.3e (%s), on the host %.3e\n", coloured.iterations,
           coloured.milliseconds, coloured.relative, coloured.converged ? "converged" : "NOT converged", resColoured);
    printf("the two solutions lie %.3e apart (max norm)\n", apart);

    spgpuDestroy(h);
    CHECK(hipGetLastError());
    const int ok = !wrong && fewLevels && natural.converged && coloured.converged && resNatural <= 10 * tol && resColoured <= 10 * tol;
    printf(ok ? "PASSED\n" : "FAILED (B differs from P A P^T, B has more levels than colours, or a solve missed its residual bound)\n");
    return ok ? 0 : 1;
}
