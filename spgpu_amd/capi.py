"""ctypes bindings of the spgpu-amd C ABI (``include/spgpu/*.h``).

Every entry point is bound with its exact C signature; nothing here computes.
Device arrays are passed as raw addresses (``tensor.data_ptr()``), scalars by
value, exactly like a C caller of the reference would (``hell.h:45-59``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPGPU_LIB") or os.path.join(_HERE, "lib", "libspgpu.so")  # SPGPU_LIB: A/B of two builds


class MissingNativeLibrary(ImportError):
    pass


if not os.path.exists(LIB_PATH):
    raise MissingNativeLibrary(
        f"{LIB_PATH} not found: build it with `make lib` (or __graft_entry__.build()); "
        "spgpu-amd has no Python or CPU fallback for its kernels")

# torch (device-memory plumbing of the tests and bench.py) ships its own HIP runtime with the
# same soname as /opt/rocm's; whichever is loaded first serves the whole process.  Load torch's
# first so that the tensors it allocates and the kernels launched here share ONE runtime.
try:
    import torch  # noqa: F401
except ImportError:  # a C-only deployment links /opt/rocm's runtime directly
    pass

lib = C.CDLL(LIB_PATH)

# ---- types ------------------------------------------------------------------
SPGPU_SUCCESS, SPGPU_UNSUPPORTED, SPGPU_UNSPECIFIED, SPGPU_OUTOFMEMORY = 0, 1, 2, 3
TYPE_INT, TYPE_FLOAT, TYPE_DOUBLE, TYPE_COMPLEX_FLOAT, TYPE_COMPLEX_DOUBLE = range(5)


class FloatComplex(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class DoubleComplex(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double)]


class HandleStruct(C.Structure):
    """Public fields of SpgpuHandleStruct (include/spgpu/core.h; reference core.h:60-82)."""
    _fields_ = [
        ("currentStream", C.c_void_p), ("defaultStream", C.c_void_p),
        ("device", C.c_int), ("warpSize", C.c_int), ("maxThreadsPerBlock", C.c_int),
        ("maxGridSizeX", C.c_int), ("maxGridSizeY", C.c_int), ("maxGridSizeZ", C.c_int),
        ("multiProcessorCount", C.c_int), ("capabilityMajor", C.c_int), ("capabilityMinor", C.c_int),
    ]


Handle = C.POINTER(HandleStruct)
ptr = C.c_void_p  # device or host address
i32 = C.c_int

# scalar C type per letter of the API
SCALAR = {"S": C.c_float, "D": C.c_double, "C": FloatComplex, "Z": DoubleComplex}
REAL = {"S": C.c_float, "D": C.c_double, "C": C.c_float, "Z": C.c_double}
TYPE_CODE = {"S": TYPE_FLOAT, "D": TYPE_DOUBLE, "C": TYPE_COMPLEX_FLOAT, "Z": TYPE_COMPLEX_DOUBLE}


def scalar(letter, value):
    """Python number -> the by-value C scalar of the given API flavour."""
    if letter in "SD":
        return SCALAR[letter](float(value))
    v = complex(value)
    return SCALAR[letter](v.real, v.imag)


def _bind(name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


DECLARED = {}  # name -> (restype, argtypes); the test suite checks it against the headers


def _decl(name, restype, argtypes):
    DECLARED[name] = (restype, argtypes)
    return _bind(name, restype, argtypes)


# ---- core.h -------------------------------------------------------------------
spgpuCreate = _decl("spgpuCreate", i32, [C.POINTER(Handle), i32])
spgpuDestroy = _decl("spgpuDestroy", None, [Handle])
spgpuStreamCreate = _decl("spgpuStreamCreate", None, [Handle, C.POINTER(C.c_void_p)])
spgpuStreamDestroy = _decl("spgpuStreamDestroy", None, [C.c_void_p])
spgpuSetStream = _decl("spgpuSetStream", None, [Handle, C.c_void_p])
spgpuGetStream = _decl("spgpuGetStream", C.c_void_p, [Handle])
spgpuSizeOf = _decl("spgpuSizeOf", C.c_size_t, [i32])

# ---- hell.h / ell.h / hdia.h ----------------------------------------------------
hellspmv, ellspmv, hdiaspmv = {}, {}, {}
axpby, maxpby, dot, mdot, nrm2, mnrm2 = {}, {}, {}, {}, {}, {}
for _L, _T in SCALAR.items():
    hellspmv[_L] = _decl(f"spgpu{_L}hellspmv", None,
                         [Handle, ptr, ptr, _T, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, ptr, _T, i32])
    ellspmv[_L] = _decl(f"spgpu{_L}ellspmv", None,
                        [Handle, ptr, ptr, _T, ptr, ptr, i32, i32, ptr, ptr, i32, i32, i32, ptr, _T, i32])
    hdiaspmv[_L] = _decl(f"spgpu{_L}hdiaspmv", None,
                         [Handle, ptr, ptr, _T, ptr, ptr, i32, ptr, i32, i32, ptr, _T])
    # ---- vector.h ---------------------------------------------------------------
    axpby[_L] = _decl(f"spgpu{_L}axpby", None, [Handle, ptr, i32, _T, ptr, _T, ptr])
    maxpby[_L] = _decl(f"spgpu{_L}maxpby", None, [Handle, ptr, i32, _T, ptr, _T, ptr, i32, i32])
    dot[_L] = _decl(f"spgpu{_L}dot", _T, [Handle, i32, ptr, ptr])
    mdot[_L] = _decl(f"spgpu{_L}mdot", None, [Handle, ptr, i32, ptr, ptr, i32, i32])
    nrm2[_L] = _decl(f"spgpu{_L}nrm2", REAL[_L], [Handle, i32, ptr])
    mnrm2[_L] = _decl(f"spgpu{_L}mnrm2", None, [Handle, ptr, i32, ptr, i32, i32])

# ---- vector.h, second half: the rest of the reference's Level-1 ----------------------
scal, vabs, axy, maxy, axypbz, maxypbz, gath, scat, setscal = {}, {}, {}, {}, {}, {}, {}, {}, {}
asum, amax, masum, mamax = {}, {}, {}, {}
for _L, _T in list(SCALAR.items()) + [("I", C.c_int)]:
    gath[_L] = _decl(f"spgpu{_L}gath", None, [Handle, ptr, i32, ptr, i32, ptr])
    scat[_L] = _decl(f"spgpu{_L}scat", None, [Handle, ptr, i32, ptr, ptr, i32, _T])
    setscal[_L] = _decl(f"spgpu{_L}setscal", None, [Handle, i32, i32, i32, _T, ptr])
    if _L == "I":
        continue
    scal[_L] = _decl(f"spgpu{_L}scal", None, [Handle, ptr, i32, _T, ptr])
    vabs[_L] = _decl(f"spgpu{_L}abs", None, [Handle, ptr, i32, _T, ptr])
    axy[_L] = _decl(f"spgpu{_L}axy", None, [Handle, ptr, i32, _T, ptr, ptr])
    maxy[_L] = _decl(f"spgpu{_L}maxy", None, [Handle, ptr, i32, _T, ptr, ptr, i32, i32])
    axypbz[_L] = _decl(f"spgpu{_L}axypbz", None, [Handle, ptr, i32, _T, ptr, _T, ptr, ptr])
    maxypbz[_L] = _decl(f"spgpu{_L}maxypbz", None, [Handle, ptr, i32, _T, ptr, _T, ptr, ptr, i32, i32])
    asum[_L] = _decl(f"spgpu{_L}asum", REAL[_L], [Handle, i32, ptr])
    amax[_L] = _decl(f"spgpu{_L}amax", REAL[_L], [Handle, i32, ptr])
    masum[_L] = _decl(f"spgpu{_L}masum", None, [Handle, ptr, i32, ptr, i32, i32])
    mamax[_L] = _decl(f"spgpu{_L}mamax", None, [Handle, ptr, i32, ptr, i32, i32])

# ---- spmm.h (new: multi-vector product of the row-sharded path) ---------------------
hellspmm, mv_interleave, mv_deinterleave = {}, {}, {}
for _L in "SD":
    _T = SCALAR[_L]
    hellspmm[_L] = _decl(f"spgpu{_L}hellspmm", None,
                         [Handle, ptr, ptr, _T, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, ptr, _T, i32, i32, i32, i32])
    mv_interleave[_L] = _decl(f"spgpu{_L}mvInterleave", None, [Handle, ptr, i32, ptr, i32, i32, i32])
    mv_deinterleave[_L] = _decl(f"spgpu{_L}mvDeinterleave", None, [Handle, ptr, i32, ptr, i32, i32, i32])

# ---- ext/spmm_mv.h: the HELL SpMM on the reference's multivector layout (vector j at base + j*pitch) ----------
hellspmm_mv = {}
for _L in "SD":
    _T = SCALAR[_L]
    hellspmm_mv[_L] = _decl(f"spgpu{_L}hellspmmMv", None,
                            [Handle, ptr, ptr, _T, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, ptr, _T, i32, i32, i32, i32])

# ---- ext/hdia_spmm.h: the HDIA and DIA SpMM on the same layout: spgpu?hdiaspmv's / spgpu?diaspmv's arguments, then
# count, pitchX, pitchYZ ----------
hdiaspmm_mv, diaspmm_mv = {}, {}
for _L in "SD":
    _T = SCALAR[_L]
    hdiaspmm_mv[_L] = _decl(f"spgpu{_L}hdiaspmmMv", None,
                            [Handle, ptr, ptr, _T, ptr, ptr, i32, ptr, i32, i32, ptr, _T, i32, i32, i32])
    diaspmm_mv[_L] = _decl(f"spgpu{_L}diaspmmMv", None,
                           [Handle, ptr, ptr, _T, ptr, ptr, i32, i32, i32, i32, ptr, _T, i32, i32, i32])

# ---- ell_conv.h / hell_conv.h / hdia_conv.h (host pointers) --------------------------
computeEllRowLenghts = _decl("computeEllRowLenghts", None, [ptr, C.POINTER(i32), i32, i32, ptr, i32])
computeEllAllocPitch = _decl("computeEllAllocPitch", i32, [i32])
cooToEll = _decl("cooToEll", None, [ptr, ptr, i32, i32, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32])
computeHellAllocSize = _decl("computeHellAllocSize", None, [C.POINTER(i32), i32, i32, ptr])
ellToHell = _decl("ellToHell", None, [ptr, ptr, ptr, i32, ptr, ptr, i32, i32, ptr, i32, i32])
getHdiaHacksCount = _decl("getHdiaHacksCount", i32, [i32, i32])
computeHdiaHackOffsetsFromCoo = _decl("computeHdiaHackOffsetsFromCoo", None,
                                      [C.POINTER(i32), ptr, i32, i32, i32, i32, ptr, ptr, i32])
cooToHdia = _decl("cooToHdia", None, [ptr, ptr, ptr, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32])


# ---- dia.h / dia_conv.h / DIA->HDIA / OELL / csput ---------------------------------
diaspmv, ellcsput = {}, {}
for _L, _T in SCALAR.items():
    diaspmv[_L] = _decl(f"spgpu{_L}diaspmv", None, [Handle, ptr, ptr, _T, ptr, ptr, i32, i32, i32, i32, ptr, _T])
    ellcsput[_L] = _decl(f"spgpu{_L}ellcsput", None, [Handle, _T, ptr, ptr, i32, i32, ptr, i32, ptr, ptr, ptr, i32])
computeDiaAllocPitch = _decl("computeDiaAllocPitch", i32, [i32])
computeDiaDiagonalsCount = _decl("computeDiaDiagonalsCount", i32, [i32, i32, i32, ptr, ptr])
coo2dia = _decl("coo2dia", None, [ptr, ptr, i32, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32])
computeHdiaHackOffsets = _decl("computeHdiaHackOffsets", None, [C.POINTER(i32), ptr, i32, ptr, i32, i32, i32, i32])
diaToHdia = _decl("diaToHdia", None, [ptr, ptr, ptr, i32, ptr, ptr, i32, i32, i32, i32])
ellToOell = _decl("ellToOell", None, [ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32, i32, i32])


# ---- convert_device.h (new: COO -> ELL / HELL in HBM) -----------------------------------------------
spgpuCooConvertWorkBytes = _decl("spgpuCooConvertWorkBytes", C.c_size_t, [i32, i32])
spgpuCooRowLengthsDevice = _decl("spgpuCooRowLengthsDevice", i32, [Handle, ptr, C.POINTER(i32), i32, i32, ptr, i32, ptr])
spgpuCooToEllDevice = _decl("spgpuCooToEllDevice", i32, [Handle, ptr, ptr, i32, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32, ptr, ptr])
spgpuHellPlanDevice = _decl("spgpuHellPlanDevice", i32, [Handle, C.POINTER(i32), ptr, i32, i32, ptr, ptr])
spgpuCooToHellDevice = _decl("spgpuCooToHellDevice", i32, [Handle, ptr, ptr, ptr, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32, ptr, ptr])
spgpuCooDiaWorkBytes = _decl("spgpuCooDiaWorkBytes", C.c_size_t, [i32, i32])
spgpuCooDiaPlanDevice = _decl("spgpuCooDiaPlanDevice", i32, [Handle, C.POINTER(i32), i32, i32, i32, ptr, ptr, i32, ptr])
spgpuCooToDiaScratchBytes = _decl("spgpuCooToDiaScratchBytes", C.c_size_t, [i32, i32])
spgpuCooToDiaDevice = _decl("spgpuCooToDiaDevice", i32, [Handle, ptr, ptr, i32, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32, ptr, ptr])
spgpuCooHdiaPlanWorkBytes = _decl("spgpuCooHdiaPlanWorkBytes", C.c_size_t, [i32, i32])
spgpuCooHdiaPlanDevice = _decl("spgpuCooHdiaPlanDevice", i32, [Handle, C.POINTER(i32), ptr, i32, i32, i32, i32, ptr, ptr, i32, ptr])
spgpuCooToHdiaScratchBytes = _decl("spgpuCooToHdiaScratchBytes", C.c_size_t, [i32, i32])
spgpuCooToHdiaDevice = _decl("spgpuCooToHdiaDevice", i32, [Handle, ptr, ptr, ptr, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32, i32, ptr, ptr])


# ---- ext/csr_device.h: CSR -> ELL / HELL in HBM, no sort and no scratch --------------------------------------------
spgpuCsrRowLengthsDevice = _decl("spgpuCsrRowLengthsDevice", i32, [Handle, ptr, C.POINTER(i32), i32, ptr, i32])
spgpuCsrToEllDevice = _decl("spgpuCsrToEllDevice", i32, [Handle, ptr, ptr, i32, i32, i32, i32, ptr, ptr, ptr, i32, i32, ptr])
spgpuCsrToHellDevice = _decl("spgpuCsrToHellDevice", i32, [Handle, ptr, ptr, ptr, i32, i32, i32, ptr, ptr, ptr, i32, i32, ptr])
# not in the headers: the two fills behind the calls above, for the A/B tool and the tests that compare them
# (..., rIdx, fill, maxBlocks): fill CSR_FILL_PLAIN (one thread per row) or CSR_FILL_TRANSPOSE (a wavefront per 32 rows,
# CSR_FILL_CHUNK slab columns per trip through LDS); maxBlocks > 0 caps the grid
CSR_FILL_PLAIN, CSR_FILL_TRANSPOSE = 0, 1
spgpuCsrToEllDeviceWith = _bind("spgpuCsrToEllDeviceWith", i32, spgpuCsrToEllDevice.argtypes + [i32, i32])
spgpuCsrToHellDeviceWith = _bind("spgpuCsrToHellDeviceWith", i32, spgpuCsrToHellDevice.argtypes + [i32, i32])
CSR_FILL_CHUNK = _bind("spgpuCsrFillChunk", i32, [])()
CSR_FILL_DEFAULT = _bind("spgpuCsrDefaultFill", i32, [])()


# ---- ext/transpose_device.h: the HELL arrays of A^T from a stored HELL or ELL matrix, in HBM -------------------------------
spgpuHellTransposeWorkBytes = _decl("spgpuHellTransposeWorkBytes", C.c_size_t, [i32, i32, i32])
# (handle, tLengths, &maxRowSize, &nonZeros, rP, hackSize, hackOffsets, rS, rIdx, rows, cols, baseIndex, slots, work)
spgpuHellTransposeLengthsDevice = _decl("spgpuHellTransposeLengthsDevice", i32,
                                        [Handle, ptr, C.POINTER(i32), C.POINTER(i32), ptr, i32, ptr, ptr, ptr, i32, i32, i32, i32, ptr])
# (handle, tValues, tIndices, tHackOffsets, tHackSize, tBaseIndex, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, cols, baseIndex,
#  slots, valuesType, tLengths, work)
spgpuHellTransposeDevice = _decl("spgpuHellTransposeDevice", i32,
                                 [Handle, ptr, ptr, ptr, i32, i32, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32, i32, i32, ptr, ptr])
# (handle, tLengths, &maxRowSize, &nonZeros, rP, ellIndicesPitch, rS, rIdx, rows, cols, baseIndex, slots, work)
spgpuEllTransposeLengthsDevice = _decl("spgpuEllTransposeLengthsDevice", i32,
                                       [Handle, ptr, C.POINTER(i32), C.POINTER(i32), ptr, i32, ptr, ptr, i32, i32, i32, i32, ptr])
# (handle, tValues, tIndices, tHackOffsets, tHackSize, tBaseIndex, cM, rP, ellValuesPitch, ellIndicesPitch, rS, rIdx, rows, cols,
#  baseIndex, slots, valuesType, tLengths, work)
spgpuEllTransposeDevice = _decl("spgpuEllTransposeDevice", i32,
                                [Handle, ptr, ptr, ptr, i32, i32, ptr, ptr, i32, i32, ptr, ptr, i32, i32, i32, i32, i32, ptr, ptr])


# ---- ext/to_csr_device.h: CSR arrays from a stored HELL or ELL matrix, in HBM ---------------------------------------------
spgpuToCsrWorkBytes = _decl("spgpuToCsrWorkBytes", C.c_size_t, [i32])
# (handle, csrRowPtr, &nonZeros, &maxRowSize, csrBaseIndex, hackSize, hackOffsets, rS, rIdx, rows, slots, work)
spgpuHellToCsrRowPtrDevice = _decl("spgpuHellToCsrRowPtrDevice", i32,
                                   [Handle, ptr, C.POINTER(i32), C.POINTER(i32), i32, i32, ptr, ptr, ptr, i32, i32, ptr])
# (handle, csrColIndices, csrValues, csrRowPtr, csrBaseIndex, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, hellBaseIndex, valuesType)
spgpuHellToCsrDevice = _decl("spgpuHellToCsrDevice", i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32])
# (handle, csrRowPtr, &nonZeros, &maxRowSize, csrBaseIndex, ellIndicesPitch, rS, rIdx, rows, slots, work)
spgpuEllToCsrRowPtrDevice = _decl("spgpuEllToCsrRowPtrDevice", i32,
                                  [Handle, ptr, C.POINTER(i32), C.POINTER(i32), i32, i32, ptr, ptr, i32, i32, ptr])
# (handle, csrColIndices, csrValues, csrRowPtr, csrBaseIndex, cM, rP, ellValuesPitch, ellIndicesPitch, rS, rIdx, rows, ellBaseIndex,
#  valuesType)
spgpuEllToCsrDevice = _decl("spgpuEllToCsrDevice", i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, i32, i32, ptr, ptr, i32, i32, i32])
# not in the headers: the two fills behind the calls above, for the A/B tool and the tests that compare them
# (..., valuesType, fill, maxBlocks): fill TO_CSR_FILL_PLAIN (one thread per storage row) or TO_CSR_FILL_TRANSPOSE (a wavefront per
# 32 storage rows, TO_CSR_FILL_CHUNK slab columns per trip through LDS); maxBlocks > 0 caps the grid
TO_CSR_FILL_PLAIN, TO_CSR_FILL_TRANSPOSE = 0, 1
spgpuHellToCsrDeviceWith = _bind("spgpuHellToCsrDeviceWith", i32, spgpuHellToCsrDevice.argtypes + [i32, i32])
spgpuEllToCsrDeviceWith = _bind("spgpuEllToCsrDeviceWith", i32, spgpuEllToCsrDevice.argtypes + [i32, i32])
TO_CSR_FILL_CHUNK = _bind("spgpuToCsrFillChunk", i32, [])()
TO_CSR_FILL_DEFAULT = _bind("spgpuToCsrDefaultFill", i32, [])()


# ---- ext/update_device.h: new coefficients for a stored HELL or ELL matrix, pattern unchanged, in HBM ------------------------
# (handle, hellValues, hackOffsets, hackSize, rows, csrRowPtr, csrValues, csrBaseIndex, valuesType, rIdx)
spgpuCsrToHellValuesDevice = _decl("spgpuCsrToHellValuesDevice", i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, i32, i32, ptr])
# (handle, ellValues, ellValuesPitch, rows, csrRowPtr, csrValues, csrBaseIndex, valuesType, rIdx)
spgpuCsrToEllValuesDevice = _decl("spgpuCsrToEllValuesDevice", i32, [Handle, ptr, i32, i32, ptr, ptr, i32, i32, ptr])
spgpuInvertRowOrderDevice = _decl("spgpuInvertRowOrderDevice", i32, [Handle, ptr, ptr, i32])
# (handle, alpha, cM, rP, hackSize, hackOffsets, rS, rowOf, rows, nnz, aI, aJ, aVal, baseIndex)
hellcsput = {}
for _L, _T in SCALAR.items():
    hellcsput[_L] = _decl(f"spgpu{_L}hellcsput", None, [Handle, _T, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, ptr, ptr, ptr, i32])
# not in the headers: the two refills behind the value calls, for the A/B tool and the tests that compare them
# (..., rIdx, fill, maxBlocks): fill UPDATE_FILL_PLAIN (one thread per row), UPDATE_FILL_TRANSPOSE (a wavefront per 32 rows through
# LDS, 16-byte stores where the slab is aligned) or < 0 for the public call's choice; maxBlocks > 0 caps the grid
UPDATE_FILL_PLAIN, UPDATE_FILL_TRANSPOSE = 0, 1
spgpuCsrToHellValuesDeviceWith = _bind("spgpuCsrToHellValuesDeviceWith", i32, spgpuCsrToHellValuesDevice.argtypes + [i32, i32])
spgpuCsrToEllValuesDeviceWith = _bind("spgpuCsrToEllValuesDeviceWith", i32, spgpuCsrToEllValuesDevice.argtypes + [i32, i32])


# ---- ext/assemble_device.h: a COO list with duplicates summed into CSR arrays, in HBM ---------------------------------------
spgpuCooAssembleWorkBytes = _decl("spgpuCooAssembleWorkBytes", C.c_size_t, [i32, i32, i32])
# (handle, &uniqueCount, csrRowPtr, perm, segPtr, rows, cols, nnz, cooRowIndices, cooColsIndices, cooBaseIndex, csrBaseIndex, work)
spgpuCooAssemblePlanDevice = _decl("spgpuCooAssemblePlanDevice", i32,
                                   [Handle, C.POINTER(i32), ptr, ptr, ptr, i32, i32, i32, ptr, ptr, i32, i32, ptr])
# (handle, csrColIndices, csrValues, uniqueCount, nnz, cooColsIndices, cooValues, cooBaseIndex, csrBaseIndex, valuesType, perm, segPtr)
spgpuCooAssembleDevice = _decl("spgpuCooAssembleDevice", i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, i32, i32, i32, ptr, ptr])
# (handle, csrValues, uniqueCount, nnz, cooValues, valuesType, perm, segPtr)
spgpuCooAssembleValuesDevice = _decl("spgpuCooAssembleValuesDevice", i32, [Handle, ptr, i32, i32, ptr, i32, ptr, ptr])
# not in the headers: the two fills behind the calls above, for the A/B tool and the tests that compare them
# (..., segPtr, fill, maxBlocks): fill ASSEMBLE_FILL_PLAIN (one thread per matrix entry), ASSEMBLE_FILL_STAGED (a workgroup per
# ASSEMBLE_TILE entries, ASSEMBLE_CHUNK positions of perm per trip through LDS, counted from the tile's first position) or < 0 for
# the public call's choice; maxBlocks > 0 caps the grid
ASSEMBLE_FILL_PLAIN, ASSEMBLE_FILL_STAGED = 0, 1
spgpuCooAssembleDeviceWith = _bind("spgpuCooAssembleDeviceWith", i32, spgpuCooAssembleDevice.argtypes + [i32, i32])
spgpuCooAssembleValuesDeviceWith = _bind("spgpuCooAssembleValuesDeviceWith", i32, spgpuCooAssembleValuesDevice.argtypes + [i32, i32])
ASSEMBLE_FILL_DEFAULT = _bind("spgpuCooAssembleDefaultFill", i32, [])()
ASSEMBLE_TILE = _bind("spgpuCooAssembleTile", i32, [])()
ASSEMBLE_CHUNK = _bind("spgpuCooAssembleChunk", i32, [])()


# ---- ext/spgemm_device.h: the sparse product C = A * B on CSR arrays with one common base, in HBM ----------------------------
spgpuCsrSpgemmWorkBytes = _decl("spgpuCsrSpgemmWorkBytes", C.c_size_t, [i32, i32, i32])
# (handle, &productsCount, aRows, aColumns, aRowPtr, aColIndices, bRowPtr, baseIndex, work)
spgpuCsrSpgemmProductsDevice = _decl("spgpuCsrSpgemmProductsDevice", i32, [Handle, C.POINTER(i32), i32, i32, ptr, ptr, ptr, i32, ptr])
# (handle, &cNonZerosCount, cRowPtr, aRows, aColumns, bColumns, aRowPtr, aColIndices, bRowPtr, bColIndices, baseIndex, productsCount, work)
spgpuCsrSpgemmPlanDevice = _decl("spgpuCsrSpgemmPlanDevice", i32,
                                 [Handle, C.POINTER(i32), ptr, i32, i32, i32, ptr, ptr, ptr, ptr, i32, i32, ptr])
# (handle, cColIndices, cValues, cNonZerosCount, aRows, aRowPtr, aColIndices, aValues, bRowPtr, bColIndices, bValues, cRowPtr, baseIndex,
#  valuesType, work)
spgpuCsrSpgemmDevice = _decl("spgpuCsrSpgemmDevice", i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32, ptr])
# (handle, cValues, aRows, aRowPtr, aColIndices, aValues, bRowPtr, bColIndices, bValues, cRowPtr, cColIndices, baseIndex, valuesType)
spgpuCsrSpgemmValuesDevice = _decl("spgpuCsrSpgemmValuesDevice", i32, [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32])
# not in the headers: the two fills behind the calls above, for the A/B tool and the tests that compare them
# (..., fill, maxBlocks): fill SPGEMM_FILL_PLAIN (one thread per entry of C), SPGEMM_FILL_STAGED (a wavefront per row of C, a row of
# at most SPGEMM_ROW_CAP entries accumulated in LDS, a longer one by the plain method) or < 0 for the public call's choice;
# maxBlocks > 0 caps the grid
SPGEMM_FILL_PLAIN, SPGEMM_FILL_STAGED = 0, 1
spgpuCsrSpgemmDeviceWith = _bind("spgpuCsrSpgemmDeviceWith", i32, spgpuCsrSpgemmDevice.argtypes + [i32, i32])
spgpuCsrSpgemmValuesDeviceWith = _bind("spgpuCsrSpgemmValuesDeviceWith", i32, spgpuCsrSpgemmValuesDevice.argtypes + [i32, i32])
SPGEMM_FILL_DEFAULT = _bind("spgpuCsrSpgemmDefaultFill", i32, [])()
SPGEMM_ROW_CAP = _bind("spgpuCsrSpgemmRowCap", i32, [])()


# ---- ext/add_device.h: the sparse sum C = alpha * A + beta * B on CSR arrays with one common base, in HBM -------------------
spgpuCsrAddWorkBytes = _decl("spgpuCsrAddWorkBytes", C.c_size_t, [i32])
# (handle, &cNonZerosCount, cRowPtr, rows, columns, aRowPtr, aColIndices, bRowPtr, bColIndices, baseIndex, work)
spgpuCsrAddPlanDevice = _decl("spgpuCsrAddPlanDevice", i32, [Handle, C.POINTER(i32), ptr, i32, i32, ptr, ptr, ptr, ptr, i32, ptr])
# (handle, cColIndices, cValues, cNonZerosCount, rows, &alpha (host), aRowPtr, aColIndices, aValues, &beta (host), bRowPtr, bColIndices,
#  bValues, cRowPtr, baseIndex, valuesType)
spgpuCsrAddDevice = _decl("spgpuCsrAddDevice", i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32])
# (handle, cValues, rows, &alpha, aRowPtr, aColIndices, aValues, &beta, bRowPtr, bColIndices, bValues, cRowPtr, baseIndex, valuesType):
# alpha and beta on the host, read at the call; in spgpuCsrAddValuesDeviceScalars in device memory, read by the kernel
spgpuCsrAddValuesDevice = _decl("spgpuCsrAddValuesDevice", i32, [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32])
spgpuCsrAddValuesDeviceScalars = _decl("spgpuCsrAddValuesDeviceScalars", i32, list(spgpuCsrAddValuesDevice.argtypes))
# not in the headers: the two fills behind the calls above, for the A/B tool and the tests that compare them
# (..., fill, maxBlocks): fill ADD_FILL_PLAIN (one thread per stored entry of A and of B, rows and ranks by bisection in global
# memory), ADD_FILL_STAGED (a workgroup per ADD_TILE entries of C, the column slices of its rows in LDS, a last row of more than
# ADD_ROW_CAP entries by the plain method) or < 0 for the public call's choice; maxBlocks > 0 caps the grid
ADD_FILL_PLAIN, ADD_FILL_STAGED = 0, 1
spgpuCsrAddDeviceWith = _bind("spgpuCsrAddDeviceWith", i32, spgpuCsrAddDevice.argtypes + [i32, i32])
spgpuCsrAddValuesDeviceWith = _bind("spgpuCsrAddValuesDeviceWith", i32, spgpuCsrAddValuesDevice.argtypes + [i32, i32])
spgpuCsrAddValuesDeviceScalarsWith = _bind("spgpuCsrAddValuesDeviceScalarsWith", i32, spgpuCsrAddValuesDevice.argtypes + [i32, i32])
ADD_FILL_DEFAULT = _bind("spgpuCsrAddDefaultFill", i32, [])()
ADD_TILE = _bind("spgpuCsrAddTile", i32, [])()
ADD_ROW_CAP = _bind("spgpuCsrAddRowCap", i32, [])()

# ---- ext/trsv_device.h: the sparse triangular solve x = T^-1 * b on CSR arrays, level-scheduled, in HBM ------------------------
TRSV_LOWER, TRSV_UPPER = 0, 1
TRSV_DIAG_STORED, TRSV_DIAG_UNIT = 0, 1
spgpuCsrTrsvWorkBytes = _decl("spgpuCsrTrsvWorkBytes", C.c_size_t, [i32])
# (handle, &levelsCount, rowOrder, levelPtr, levelPtrHost (host), rows, rowPtr, colIndices, baseIndex, side, diag, work)
spgpuCsrTrsvPlanDevice = _decl("spgpuCsrTrsvPlanDevice", i32, [Handle, C.POINTER(i32), ptr, ptr, C.POINTER(i32), i32, ptr, ptr, i32, i32, i32, ptr])
# (handle, x, b, rows, levelsCount, rowOrder, levelPtr, levelPtrHost (host), rowPtr, colIndices, values, baseIndex, side, diag, valuesType)
spgpuCsrTrsvDevice = _decl("spgpuCsrTrsvDevice", i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, C.POINTER(i32), ptr, ptr, ptr, i32, i32, i32, i32])
# not in the headers: the two solves behind the call above, for the A/B tool and the tests that compare them
# (..., solve, maxBlocks): solve TRSV_SOLVE_PLAIN (one launch per level), TRSV_SOLVE_CHAINED (a run of levels of at most
# TRSV_CHAIN_WIDTH rows each is one launch of one workgroup) or < 0 for the public call's choice; maxBlocks > 0 caps a level's grid
TRSV_SOLVE_PLAIN, TRSV_SOLVE_CHAINED = 0, 1
spgpuCsrTrsvDeviceWith = _bind("spgpuCsrTrsvDeviceWith", i32, spgpuCsrTrsvDevice.argtypes + [i32, i32])
TRSV_SOLVE_DEFAULT = _bind("spgpuCsrTrsvDefaultSolve", i32, [])()
TRSV_CHAIN_WIDTH = _bind("spgpuCsrTrsvChainWidth", i32, [])()

# ---- ext/ilu0_device.h: the incomplete factorisation ILU(0) on CSR arrays, level-scheduled, in HBM ------------------------------
spgpuCsrIlu0WorkBytes = _decl("spgpuCsrIlu0WorkBytes", C.c_size_t, [i32])
# (handle, &levelsCount, rowOrder, levelPtr, levelPtrHost (host, rows + 2 ints), diagPos, rows, rowPtr, colIndices, baseIndex, work)
spgpuCsrIlu0PlanDevice = _decl("spgpuCsrIlu0PlanDevice", i32, [Handle, C.POINTER(i32), ptr, ptr, C.POINTER(i32), ptr, i32, ptr, ptr, i32, ptr])
# (handle, luValues, aValues, rows, levelsCount, rowOrder, levelPtr, levelPtrHost (host), diagPos, rowPtr, colIndices, baseIndex, valuesType)
spgpuCsrIlu0Device = _decl("spgpuCsrIlu0Device", i32, [Handle, ptr, ptr, i32, i32, ptr, ptr, C.POINTER(i32), ptr, ptr, ptr, i32, i32])
# not in the headers: the row shapes and segmentings behind the call above, for the A/B tool and the tests that compare them
# (..., shape, solve, maxBlocks): shape ILU0_SHAPE_THREAD (one thread per row), a power of two in [2, 64] (that many lanes of one
# wavefront per row) or <= 0 for the public call's choice, csr_ilu0_default_shape(rows, nnz); solve TRSV_SOLVE_PLAIN (one launch per
# level), TRSV_SOLVE_CHAINED (a run of levels of at most ILU0_CHAIN_WIDTH rows each is one launch of one workgroup) or < 0 for the
# public call's choice; maxBlocks > 0 caps a level's grid
ILU0_SHAPE_THREAD = 1
spgpuCsrIlu0DeviceWith = _bind("spgpuCsrIlu0DeviceWith", i32, spgpuCsrIlu0Device.argtypes + [i32, i32, i32])
csr_ilu0_default_shape = _bind("spgpuCsrIlu0DefaultShape", i32, [i32, i32])
ILU0_SOLVE_DEFAULT = _bind("spgpuCsrIlu0DefaultSolve", i32, [])()
ILU0_CHAIN_WIDTH = _bind("spgpuCsrIlu0ChainWidth", i32, [])()
# the two GROUP widths the rule can choose, and the mean row lengths up to which THREAD and the narrow GROUP run
ILU0_GROUP_NARROW, ILU0_GROUP_WIDE, ILU0_THREAD_MAX_MEAN, ILU0_NARROW_MAX_MEAN = (
    _bind("spgpuCsrIlu0ShapeConstant", i32, [i32])(k) for k in range(4))
ILU0_SHAPES = (ILU0_SHAPE_THREAD, ILU0_GROUP_NARROW, ILU0_GROUP_WIDE)

# ---- ext/aggregate_device.h: strength of connection, MIS-2 aggregates and the tentative prolongator on CSR arrays, in HBM -----------
spgpuCsrAggregateWorkBytes = _decl("spgpuCsrAggregateWorkBytes", C.c_size_t, [i32])
# (handle, strong (bytes, one per entry), diagAbs, rows, rowPtr, colIndices, values, baseIndex, theta, valuesType)
spgpuCsrStrengthDevice = _decl("spgpuCsrStrengthDevice", i32, [Handle, ptr, ptr, i32, ptr, ptr, ptr, i32, C.c_double, i32])
# (handle, &aggregatesCount, &roundsCount, aggregateOf, aggregateSize, rows, rowPtr, colIndices, strong or NULL, baseIndex, work)
spgpuCsrAggregateDevice = _decl("spgpuCsrAggregateDevice", i32, [Handle, C.POINTER(i32), C.POINTER(i32), ptr, ptr, i32, ptr, ptr, ptr, i32,
                                                                ptr])
# (handle, tRowPtr, tColIndices, tValues, rows, aggregateOf, candidate or NULL, baseIndex, valuesType)
spgpuCsrTentativeDevice = _decl("spgpuCsrTentativeDevice", i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, i32, i32])
# not in the headers: the row shapes behind the calls above, for the A/B tool and the tests that compare them
# (..., shape, maxBlocks): shape AGG_SHAPE_THREAD (one thread per row), a power of two in [2, 64] (that many lanes of one wavefront
# per row) or <= 0 for the public call's choice -- csr_aggregate_default_shape(rows, nnz) for the aggregation, one thread per row for
# the strength call, which cannot read nnz without a synchronise; maxBlocks > 0 caps the grids
AGG_SHAPE_THREAD = 1
spgpuCsrAggregateDeviceWith = _bind("spgpuCsrAggregateDeviceWith", i32, spgpuCsrAggregateDevice.argtypes + [i32, i32])
spgpuCsrStrengthDeviceWith = _bind("spgpuCsrStrengthDeviceWith", i32, spgpuCsrStrengthDevice.argtypes + [i32, i32])
csr_aggregate_default_shape = _bind("spgpuCsrAggregateDefaultShape", i32, [i32, i32])

# ---- ext/colour_device.h: multicolour ordering on CSR arrays -- colouring, order, symmetric permutation -- in HBM ---------------------
spgpuCsrColourWorkBytes = _decl("spgpuCsrColourWorkBytes", C.c_size_t, [i32])
# (handle, &coloursCount, &roundsCount, colourOf, rows, rowPtr, colIndices, baseIndex, work)
spgpuCsrColourDevice = _decl("spgpuCsrColourDevice", i32, [Handle, C.POINTER(i32), C.POINTER(i32), ptr, i32, ptr, ptr, i32, ptr])
# (handle, order, inverse, colourPtr, rows, coloursCount, colourOf, work)
spgpuCsrColourOrderDevice = _decl("spgpuCsrColourOrderDevice", i32, [Handle, ptr, ptr, ptr, i32, i32, ptr, ptr])
spgpuCsrPermuteWorkBytes = _decl("spgpuCsrPermuteWorkBytes", C.c_size_t, [i32])
# (handle, bRowPtr, bColIndices, bValues, rows, order, inverse, aRowPtr, aColIndices, aValues, baseIndex, valuesType, work)
spgpuCsrPermuteDevice = _decl("spgpuCsrPermuteDevice", i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, ptr, ptr, ptr, i32, i32, ptr])
# not in the headers: the row shapes behind the calls above, for the A/B tool and the tests that compare them
# (..., shape, maxBlocks): shape COLOUR_SHAPE_THREAD (one thread per row), a power of two in [2, 64] (that many lanes of one wavefront
# per row) or <= 0 for the public call's choice -- csr_colour_default_shape(rows, nnz) for the colouring, one fixed shape for the
# permutation, which cannot read nnz without a synchronise; maxBlocks > 0 caps the grids
COLOUR_SHAPE_THREAD = 1
spgpuCsrColourDeviceWith = _bind("spgpuCsrColourDeviceWith", i32, spgpuCsrColourDevice.argtypes + [i32, i32])
spgpuCsrPermuteDeviceWith = _bind("spgpuCsrPermuteDeviceWith", i32, spgpuCsrPermuteDevice.argtypes + [i32, i32])
csr_colour_default_shape = _bind("spgpuCsrColourDefaultShape", i32, [i32, i32])

# ---- ext/sweep_device.h: multicolour Gauss-Seidel / SOR sweeps in place and the residual r = b - A x on CSR arrays, in HBM ------------
SWEEP_FORWARD, SWEEP_BACKWARD, SWEEP_SYMMETRIC = 0, 1, 2
spgpuCsrSweepWorkBytes = _decl("spgpuCsrSweepWorkBytes", C.c_size_t, [i32])
# (handle, &entriesCount, diagPos, colourPtrHost (host), rows, coloursCount, order or NULL, colourPtr, colourOf, rowPtr, colIndices,
#  baseIndex, work)
spgpuCsrSweepPlanDevice = _decl("spgpuCsrSweepPlanDevice", i32, [Handle, C.POINTER(i32), ptr, C.POINTER(i32), i32, i32, ptr, ptr, ptr, ptr, ptr,
                                                                i32, ptr])
# (handle, x, b, rows, coloursCount, order or NULL, colourPtrHost (host), diagPos, rowPtr, colIndices, values, baseIndex, direction,
#  omega (host, one element, or NULL), valuesType, entriesCount)
spgpuCsrSweepDevice = _decl("spgpuCsrSweepDevice", i32, [Handle, ptr, ptr, i32, i32, ptr, C.POINTER(i32), ptr, ptr, ptr, ptr, i32, i32, ptr, i32,
                                                        i32])
# (handle, r, b, x, rows, rowPtr, colIndices, values, baseIndex, valuesType, entriesCount)
spgpuCsrResidualDevice = _decl("spgpuCsrResidualDevice", i32, [Handle, ptr, ptr, ptr, i32, ptr, ptr, ptr, i32, i32, i32])
# not in the headers: the row shapes and segmentings behind the calls above, for the A/B tool and the tests that compare them
# (..., shape, solve, maxBlocks) and (..., shape, maxBlocks): shape SWEEP_SHAPE_THREAD (one thread per row), a power of two in [2, 64]
# (that many lanes of one wavefront per row) or <= 0 for the public call's choice, csr_sweep_default_shape(rows, nnz); solve
# TRSV_SOLVE_PLAIN (one launch per colour), TRSV_SOLVE_CHAINED (a run of colours of at most SWEEP_CHAIN_WIDTH rows each is one launch
# of one workgroup per SWEEP_CHAIN_PASSES colours) or < 0 for the public call's choice; maxBlocks > 0 caps a grid-strided launch
SWEEP_SHAPE_THREAD = 1
spgpuCsrSweepDeviceWith = _bind("spgpuCsrSweepDeviceWith", i32, spgpuCsrSweepDevice.argtypes + [i32, i32, i32])
spgpuCsrResidualDeviceWith = _bind("spgpuCsrResidualDeviceWith", i32, spgpuCsrResidualDevice.argtypes + [i32, i32])
csr_sweep_default_shape = _bind("spgpuCsrSweepDefaultShape", i32, [i32, i32])
SWEEP_SOLVE_DEFAULT = _bind("spgpuCsrSweepDefaultSolve", i32, [])()
SWEEP_CHAIN_WIDTH = _bind("spgpuCsrSweepChainWidth", i32, [])()
SWEEP_CHAIN_PASSES = _bind("spgpuCsrSweepChainPasses", i32, [])()
# (colourPtrHost (host), coloursCount, direction, solve) -> the launches of one sweep call
csr_sweep_launches = _bind("spgpuCsrSweepLaunches", i32, [C.POINTER(i32), i32, i32, i32])


# ---- oell_device.h (new: rows ordered by length in HBM) + the host order (ell_conv.h) ----------------------------
oellOrder = _decl("oellOrder", None, [ptr, ptr, ptr, i32, i32, i32])
oellOrderAligned = _decl("oellOrderAligned", None, [ptr, ptr, ptr, i32, i32, i32])
spgpuOellOrderWorkBytes = _decl("spgpuOellOrderWorkBytes", C.c_size_t, [i32])
spgpuOellOrderDevice = _decl("spgpuOellOrderDevice", i32, [Handle, ptr, ptr, ptr, i32, i32, i32, ptr])
spgpuOellOrderAlignedDevice = _decl("spgpuOellOrderAlignedDevice", i32, [Handle, ptr, ptr, ptr, i32, i32, i32, ptr])
spgpuEllToOellDevice = _decl("spgpuEllToOellDevice", i32, [Handle, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32, i32, i32, i32, i32, ptr])
spgpuCooPermuteRowsDevice = _decl("spgpuCooPermuteRowsDevice", i32, [Handle, ptr, ptr, i32, ptr, i32, i32, ptr])


# ---- sharded.h (new: the row-sharded SpMM driver in C, RCCL through dlopen) ----------------------------------------
class HellBlockD(C.Structure):
    """spgpuHellBlockD: one HELL row block in device memory."""
    _fields_ = [("cM", C.c_void_p), ("rP", C.c_void_p), ("hackSize", C.c_int), ("hackOffsets", C.c_void_p), ("rS", C.c_void_p),
                ("rows", C.c_int), ("avgNnzPerRow", C.c_int), ("baseIndex", C.c_int), ("slots", C.c_longlong)]


EXCHANGE_ALLGATHER, EXCHANGE_NEEDED = 0, 1
ShardedPlan = C.c_void_p
spgpuCommAvailable = _decl("spgpuCommAvailable", i32, [])
spgpuCommGetUniqueId = _decl("spgpuCommGetUniqueId", i32, [ptr])
spgpuCommInitRank = _decl("spgpuCommInitRank", i32, [C.POINTER(C.c_void_p), i32, ptr, i32])
spgpuCommInitAll = _decl("spgpuCommInitAll", i32, [C.POINTER(C.c_void_p), i32, ptr])
spgpuCommDestroy = _decl("spgpuCommDestroy", None, [ptr])
spgpuDhellspmmShardedCreate = _decl("spgpuDhellspmmShardedCreate", i32,
                                    [C.POINTER(ShardedPlan), Handle, ptr, i32, i32, C.POINTER(C.c_longlong), C.POINTER(HellBlockD),
                                     C.POINTER(HellBlockD), i32, i32])
spgpuDhellspmmShardedStep = _decl("spgpuDhellspmmShardedStep", i32, [ShardedPlan, ptr, ptr, C.c_double, ptr, C.c_double])
spgpuDhellspmmShardedExchange = _decl("spgpuDhellspmmShardedExchange", i32, [ShardedPlan, ptr])
spgpuDhellspmmShardedExchangeWait = _decl("spgpuDhellspmmShardedExchangeWait", i32, [ShardedPlan])
spgpuDhellspmmShardedProducts = _decl("spgpuDhellspmmShardedProducts", i32, [ShardedPlan, ptr, ptr, C.c_double, ptr, C.c_double])
spgpuDhellspmmShardedRowsReceived = _decl("spgpuDhellspmmShardedRowsReceived", C.c_longlong, [ShardedPlan])
spgpuDhellspmmShardedExchanged = _decl("spgpuDhellspmmShardedExchanged", C.c_void_p, [ShardedPlan, C.POINTER(C.c_longlong)])
spgpuDhellspmmShardedDestroy = _decl("spgpuDhellspmmShardedDestroy", None, [ShardedPlan])


def hell_block(part, avg_nnz=0):
    """A device HELL dict (cM, rP, hack_offsets, rS tensors; rows, hack_size) as the C struct; keep `part` alive."""
    p = lambda t: t.data_ptr()
    slots = int(part["slots"]) if "slots" in part else int(part["cM"].numel())
    return HellBlockD(p(part["cM"]), p(part["rP"]), part["hack_size"], p(part["hack_offsets"]), p(part["rS"]), part["rows"], avg_nnz,
                      part.get("base", 0), slots)


# ---- mmread.h (C wrappers of the Matrix Market reader) --------------------------------------------------------
spgpuMmProperties = _decl("spgpuMmProperties", i32, [C.c_char_p, ptr])
spgpuMmReadCoo = _decl("spgpuMmReadCoo", i32, [C.c_char_p, C.c_char, ptr, ptr, ptr])
spgpuMmUnfoldedSizeD = _decl("spgpuMmUnfoldedSizeD", i32, [ptr, ptr, ptr, i32])
spgpuMmUnfoldD = _decl("spgpuMmUnfoldD", None, [ptr, ptr, ptr, ptr, ptr, ptr, i32])


# ---- device_scalars.h (new: results and coefficients in device memory, graph-capturable) ---------------------
dot_device, axpby_device, axpby_quot_device, div_device, nrm2_device = {}, {}, {}, {}, {}
for _L in "SD":
    dot_device[_L] = _decl(f"spgpu{_L}dotDevice", None, [Handle, ptr, i32, ptr, ptr])
    nrm2_device[_L] = _decl(f"spgpu{_L}nrm2Device", None, [Handle, ptr, i32, ptr])
    axpby_device[_L] = _decl(f"spgpu{_L}axpbyDevice", None, [Handle, ptr, i32, ptr, ptr, ptr, ptr])
    axpby_quot_device[_L] = _decl(f"spgpu{_L}axpbyQuotDevice", None, [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, i32, ptr])
    div_device[_L] = _decl(f"spgpu{_L}divDevice", None, [Handle, ptr, ptr, ptr, i32])
hellspmv_dot_device, axpby_pair_dot_device = {}, {}
for _L in "SD":
    _S = SCALAR[_L]
    hellspmv_dot_device[_L] = _decl(f"spgpu{_L}hellspmvDotDevice", None,
                                    [Handle, ptr, ptr, ptr, ptr, _S, ptr, ptr, i32, ptr, ptr, i32, ptr, _S, i32])
    axpby_pair_dot_device[_L] = _decl(f"spgpu{_L}axpbyPairDotDevice", None,
                                      [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr])


# ---- ext/device_scalars_mv.h: the same on pitch multivectors, one result / coefficient per vector (arrays of `count` elements);
# count and pitch follow the single-vector argument list ----------
mdot_device, mnrm2_device, mdiv_device = {}, {}, {}
maxpby_device, maxpby_quot_device, maxpby_pair_dot_device = {}, {}, {}
for _L in "SD":
    mdot_device[_L] = _decl(f"spgpu{_L}mdotDevice", None, [Handle, ptr, i32, ptr, ptr, i32, i32])
    mnrm2_device[_L] = _decl(f"spgpu{_L}mnrm2Device", None, [Handle, ptr, i32, ptr, i32, i32])
    mdiv_device[_L] = _decl(f"spgpu{_L}mdivDevice", None, [Handle, ptr, ptr, ptr, i32, i32])
    maxpby_device[_L] = _decl(f"spgpu{_L}maxpbyDevice", None, [Handle, ptr, i32, ptr, ptr, ptr, ptr, i32, i32])
    maxpby_quot_device[_L] = _decl(f"spgpu{_L}maxpbyQuotDevice", None,
                                   [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, i32, ptr, i32, i32])
    maxpby_pair_dot_device[_L] = _decl(f"spgpu{_L}maxpbyPairDotDevice", None,
                                       [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32])

# ---- ext/precond.h: the diagonal of a matrix the library holds (the matrix arguments lead as in the matching spmv), and the Jacobi
# step of PCG fused into the device-scalar calls; the m-forms take the single-vector argument lists, then count and pitch ----------
hell_diag, ell_diag, hdia_diag = {}, {}, {}
axy_dot_device, axpby_pair_axy_dot_device, maxy_dot_device, maxpby_pair_axy_dot_device = {}, {}, {}, {}
for _L in "SD":
    hell_diag[_L] = _decl(f"spgpu{_L}hellDiag", None, [Handle, ptr, ptr, ptr, i32, ptr, ptr, i32, i32, i32])
    ell_diag[_L] = _decl(f"spgpu{_L}ellDiag", None, [Handle, ptr, ptr, ptr, i32, i32, ptr, i32, i32, i32, i32])
    hdia_diag[_L] = _decl(f"spgpu{_L}hdiaDiag", None, [Handle, ptr, ptr, ptr, i32, ptr, i32, i32, i32])
    axy_dot_device[_L] = _decl(f"spgpu{_L}axyDotDevice", None, [Handle, ptr, i32, ptr, ptr, ptr])
    axpby_pair_axy_dot_device[_L] = _decl(f"spgpu{_L}axpbyPairAxyDotDevice", None,
                                          [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr])
    maxy_dot_device[_L] = _decl(f"spgpu{_L}maxyDotDevice", None, [Handle, ptr, i32, ptr, ptr, ptr, i32, i32])
    maxpby_pair_axy_dot_device[_L] = _decl(f"spgpu{_L}maxpbyPairAxyDotDevice", None,
                                           [Handle, ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, i32, i32])

# ---- ext/hdia_solver.h: the fused SpMV + dot of a captured CG iteration on HDIA / DIA: result, w, then spgpu?hdiaspmv's /
# spgpu?diaspmv's arguments ----------
hdiaspmv_dot_device, diaspmv_dot_device = {}, {}
for _L in "SD":
    _S = SCALAR[_L]
    hdiaspmv_dot_device[_L] = _decl(f"spgpu{_L}hdiaspmvDotDevice", None,
                                    [Handle, ptr, ptr, ptr, ptr, _S, ptr, ptr, i32, ptr, i32, i32, ptr, _S])
    diaspmv_dot_device[_L] = _decl(f"spgpu{_L}diaspmvDotDevice", None,
                                   [Handle, ptr, ptr, ptr, ptr, _S, ptr, ptr, i32, i32, i32, i32, ptr, _S])

# ---- tuning.h: per-handle kernel-form hint ---------------------------------------------------------------------
FORM_AUTO, FORM_GATHER, FORM_STRIPS, FORM_XTILE, FORM_SWEEP = range(5)
spgpuSetSpmvForm = _decl("spgpuSetSpmvForm", None, [Handle, i32])
spgpuGetSpmvForm = _decl("spgpuGetSpmvForm", i32, [Handle])
spgpuDeepListOverflows = _decl("spgpuDeepListOverflows", i32, [Handle])
spgpuDeepListFallbacks = _decl("spgpuDeepListFallbacks", i32, [Handle])
spgpuDeepListsRecycled = _decl("spgpuDeepListsRecycled", i32, [Handle])
spgpuSpmvPlanCounts = _decl("spgpuSpmvPlanCounts", None, [Handle, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)])
spgpuHellSpmvPrepare = _decl("spgpuHellSpmvPrepare", i32, [Handle, i32, ptr, ptr, i32, ptr, ptr, ptr, i32, i32])
spgpuHellSpmvFreeze = _decl("spgpuHellSpmvFreeze", i32, [Handle, i32, ptr, ptr, i32, ptr, ptr, ptr, i32, i32])
spgpuEllSpmvFreeze = _decl("spgpuEllSpmvFreeze", i32, [Handle, i32, ptr, ptr, i32, i32, ptr, ptr, i32, i32, i32])
spgpuHellSpmvAdopt = _decl("spgpuHellSpmvAdopt", i32, [Handle, i32, ptr, ptr, i32, ptr, ptr, i32, i32])
spgpuEllSpmvAdopt = _decl("spgpuEllSpmvAdopt", i32, [Handle, i32, ptr, ptr, i32, i32, ptr, i32, i32, i32])
spgpuHellSpmvOptimize = _decl("spgpuHellSpmvOptimize", i32, [Handle, i32, ptr, ptr, i32, ptr, ptr, ptr, i32, i32])
SPMV_AS_IS, SPMV_FROZEN, SPMV_ADOPTED = 0, 1, 2
spgpuSpmvAdoptedUses = _decl("spgpuSpmvAdoptedUses", i32, [Handle])
spgpuSpmvThaw = _decl("spgpuSpmvThaw", i32, [Handle, ptr])
spgpuSpmvFrozenBytes = _decl("spgpuSpmvFrozenBytes", C.c_longlong, [Handle])
spgpuEllSpmvPrepare = _decl("spgpuEllSpmvPrepare", i32, [Handle, i32, ptr, ptr, i32, i32, ptr, ptr, i32, i32, i32])

# ---- ext/graph.h: holds that let captured graphs use a matrix' records ---------------------------------------
SPGPU_IN_USE = 4  # spgpuSpmvThaw refused: a hold is on the matrix
spgpuSpmvHold = _decl("spgpuSpmvHold", i32, [Handle, ptr])
spgpuSpmvRelease = _decl("spgpuSpmvRelease", i32, [Handle, ptr])
spgpuSpmvHolds = _decl("spgpuSpmvHolds", i32, [Handle, ptr])


def plan_counts(handle):
    """(launches with a plan, analyses started, plans found stale) of the handle's ordered ELL/HELL SpMVs (tuning.h)."""
    u, b, s = i32(0), i32(0), i32(0)
    spgpuSpmvPlanCounts(handle, C.byref(u), C.byref(b), C.byref(s))
    return u.value, b.value, s.value
spgpuGetLastSpmvForm = _decl("spgpuGetLastSpmvForm", i32, [Handle])
# which queue kernel the last call launched on the ordered path (0: it took another path): sub-groups per workgroup | flags
ORDERED_SUBS_MASK, ORDERED_PLAN, ORDERED_PACKED, ORDERED_DEEP = 0xFF, 0x100, 0x200, 0x400
spgpuGetLastOrderedLaunch = _decl("spgpuGetLastOrderedLaunch", i32, [Handle])
spgpuTuningVariantsBuilt = _decl("spgpuTuningVariantsBuilt", i32, [])
spgpuHellSpmvForm = _decl("spgpuHellSpmvForm", i32, [Handle, i32, ptr, i32, ptr, ptr, i32, i32])
spgpuEllSpmvForm = _decl("spgpuEllSpmvForm", i32, [Handle, i32, ptr, i32, ptr, i32, i32, i32])

# ---- tuning.h: environment knobs are cached by the library; call after changing one ---------------------------
spgpuTuningReload = _decl("spgpuTuningReload", None, [])


def create_handle(device=0):
    h = Handle()
    status = spgpuCreate(C.byref(h), device)
    if status != SPGPU_SUCCESS or not h:
        raise RuntimeError(f"spgpuCreate(device={device}) failed with status {status}")
    return h
