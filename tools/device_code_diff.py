#!/usr/bin/env python3
"""Is the device code of two builds of libspgpu.so the same?  Takes the gfx950 code objects out of each library's fat binary
(one per translation unit), and compares, kernel by kernel over the union of all of them: the set of kernel symbols, every
kernel's instruction stream (llvm-objdump -d without addresses and encodings; branches print as relative offsets, so the text
does not depend on where a kernel sits) and its resource note (VGPRs, SGPRs, LDS, scratch, kernarg size).  The fill between a
kernel's last instruction and the next kernel or the end of the section (s_nop 0 or zero words, which the disassembler prints under
the kernel in front of them) is not compared: it depends on which kernel comes next, not on the kernel.
usage: tools/device_code_diff.py OLD/libspgpu.so NEW/libspgpu.so [-v] [OLDSYMBOL=NEWSYMBOL ...]   (exit status 1 if anything
differs; a kernel that was renamed is compared under its new name)"""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FILL = ("s_nop 0", "v_cndmask_b32_e32 v0, s0, v0, vcc", "...")  # the second is how a zero word disassembles
NOTE_KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")


def code_objects(library, tmp):
    """The gfx950 ELF of every bundle in the library's .hip_fatbin section."""
    fatbin = os.path.join(tmp, "fatbin")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fatbin}", library, os.path.join(tmp, "copy")], check=True)
    data = open(fatbin, "rb").read()
    at = data.find(MAGIC)
    while at >= 0:
        entries, = struct.unpack_from("<Q", data, at + len(MAGIC))
        cursor = at + len(MAGIC) + 8
        for _ in range(entries):
            offset, size, id_size = struct.unpack_from("<QQQ", data, cursor)
            target = data[cursor + 24:cursor + 24 + id_size].decode()
            cursor += 24 + id_size
            if "gfx950" in target and size:
                yield data[at + offset:at + offset + size]
        at = data.find(MAGIC, at + 1)


def kernels_of(library):
    """{kernel symbol: [(instruction text, resource tuple) per code object that holds it]} over the whole library."""
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n, elf in enumerate(code_objects(library, tmp)):
            path = os.path.join(tmp, f"co{n}.elf")
            open(path, "wb").write(elf)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
            resources = {}
            for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                get = lambda key: re.search(rf"\.{key}:\s+(\S+)", block).group(1)
                resources[get("name")] = tuple(get(key) for key in NOTE_KEYS)
            listing = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", path],
                                     capture_output=True, text=True, check=True).stdout
            name, lines, compared = None, [], 0
            for line in listing.split("\n") + ["<end>:"]:
                label = re.match(r"^<?([^\s<>]+)>?:$", line.strip()) if not line.startswith((" ", "\t")) else None
                if label:
                    while lines and lines[-1] in FILL:
                        lines.pop()
                    if name in resources:
                        found.setdefault(name, []).append(("\n".join(lines), resources[name]))  # (a template: one per unit)
                        compared += 1
                    elif name is not None and lines:
                        sys.exit(f"{library}: code under the label {name} belongs to no kernel of the resource notes: not compared")
                    name, lines = label.group(1), []
                elif line.strip():
                    lines.append(re.sub(r"\s*//.*$", "", line).strip())
            if compared != len(resources):
                sys.exit(f"{library}: {len(resources)} kernels in the notes of a code object, {compared} of them found in its disassembly")
    return {name: sorted(copies) for name, copies in found.items()}


def main():
    old, new = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    for was, now in (arg.split("=") for arg in sys.argv[3:] if "=" in arg):
        old.setdefault(now, []).extend(old.pop(was))
        print(f"renamed: {was} -> {now}")
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = [k for k in sorted(set(old) & set(new)) if set(old[k]) != set(new[k])]  # a kernel of a header: a copy per unit
    instructions = sum(len(text.split("\n")) for copies in new.values() for text, _ in copies)
    print(f"kernels compared: {len(set(old) & set(new))} (old {len(old)}, new {len(new)}); {instructions} instructions in the new build")
    print(f"compared per kernel: instruction stream, {', '.join(NOTE_KEYS)}")
    print(f"only in old: {len(gone)}  only in new: {len(added)}  differing: {len(differ)}")
    for title, names in (("only in old", gone), ("only in new", added), ("differing", differ)):
        for k in names:
            print(f"  {title}: {k}")
    if "-v" in sys.argv:
        for k in sorted(new):
            print("  same:", " ".join(new[k][0][1]), k)
    return 1 if gone or added or differ else 0


if __name__ == "__main__":
    sys.exit(main())
