"""Diff the gfx950 machine code of named kernels between two builds of libgslic_hip.so (CPU only: llvm-objdump).

    python tools/kernel_disasm_diff.py OLD.so NEW.so [--match REGEX] [--list]

Every offload bundle in the libraries' .hip_fatbin section is split out (the bundle header is parsed here), its gfx950 code objects are
disassembled with llvm-objdump, and the instruction stream of each kernel symbol that matches REGEX (default: every kernel symbol present in
OLD.so) is compared with NEW.so's.  Addresses, encodings, comments, the alignment padding behind a kernel and the pc-relative distances to
constants are dropped and branch targets are made relative to the symbol, so a kernel that only moved inside its code object compares equal.
Prints one line per differing or missing kernel and exits 1 if there is any.  The colour-only kernels of a change that adds a variant are checked
with the default (all kernels of OLD.so)."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    """The gfx950 code objects (ELF bytes) of every offload bundle in `lib`."""
    data = open(lib, "rb").read()
    out, pos = [], 0
    while True:
        pos = data.find(MAGIC, pos)
        if pos < 0:
            return out
        n = struct.unpack_from("<Q", data, pos + 24)[0]
        q = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[pos + off:pos + off + size])
        pos += len(MAGIC)


def kernels(lib):
    """{symbol: [normalised instruction lines]} over all code objects of `lib`."""
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for i, co in enumerate(code_objects(lib)):
            path = os.path.join(td, f"co{i}.elf")
            open(path, "wb").write(co)
            txt = subprocess.run([os.path.join(ROCM_LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", path],
                                 capture_output=True, text=True, check=True).stdout
            cur = None
            for line in txt.splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line.strip())
                if m:
                    cur = m.group(1)
                    res[cur] = []
                    continue
                if cur is None or not line.strip():
                    continue
                ins = line.split("//")[0].strip()
                ins = re.sub(r"<[^>]*\+(0x[0-9a-f]+)>", r"<+\1>", ins)   # branch target: offset inside the symbol only
                ins = re.sub(r"\b0x[0-9a-f]+ <", "<", ins)
                if ins and res[cur] and res[cur][-1].startswith("s_getpc_b64"):
                    ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)   # (the distance to a constant moves with the code object's layout)
                if ins:
                    res[cur].append(ins)
    for k, v in res.items():   # the s_nop / s_code_end padding up to the next symbol's alignment
        while v and (v[-1].startswith("s_nop") or v[-1].startswith("s_code_end")):
            v.pop()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--match", default=None, help="regex on the (mangled) symbol; default: every kernel of OLD")
    ap.add_argument("--list", action="store_true", help="also print the kernels that compare equal")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    names = sorted(k for k in old if (re.search(a.match, k) if a.match else True) and not k.startswith("__"))
    bad = 0
    for k in names:
        if k not in new:
            print(f"MISSING {k}")
            bad += 1
        elif old[k] != new[k]:
            print(f"DIFFERS {k} ({len(old[k])} -> {len(new[k])} instructions)")
            bad += 1
        elif a.list:
            print(f"same    {k} ({len(old[k])} instructions)")
    print(f"{len(names)} kernels compared, {bad} differ", file=sys.stderr)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
