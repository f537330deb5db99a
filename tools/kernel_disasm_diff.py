"""Compares the gfx950 kernels of two builds of libsjpeg_amd.so: every kernel symbol that exists in both is
disassembled and compared instruction by instruction, pc-relative operands (branch targets, the literals of the
s_add_u32 / s_addc_u32 pair directly behind an s_getpc_b64) and addresses masked; the alignment padding behind a
kernel's last instruction (s_nop, s_code_end, objdump's "..." for a run of them) is not part of it -- how much there is
depends on what follows the kernel in its code object, and a kernel may move to another one.  Needs no GPU:

    python tools/kernel_disasm_diff.py OLD/libsjpeg_amd.so NEW/libsjpeg_amd.so > profiles/r09/packed_disasm.txt

Exit status 1 when a kernel that exists in both builds differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")


def code_objects(lib, tmp, tag):
    """The gfx950 code objects bundled into the library's .hip_fatbin section."""
    fat = os.path.join(tmp, tag + ".fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    blob = open(fat, "rb").read()
    out, at, k = [], 0, 0
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    while True:
        at = blob.find(magic, at)
        if at < 0:
            break
        end = blob.find(magic, at + 1)
        part = os.path.join(tmp, f"{tag}.{k}.bundle")
        open(part, "wb").write(blob[at:end if end > 0 else len(blob)])
        co = os.path.join(tmp, f"{tag}.{k}.co")
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                               f"--output={co}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"])
        if os.path.getsize(co) > 0:
            out.append(co)
        at += 1
        k += 1
    return out


MASKS = [
    (re.compile(r"^\s*[0-9a-f]+:\s*"), ""),                                  # address column (objdump --no-show-raw-insn -> none)
    (re.compile(r"//.*$"), ""),                                              # encoding / address comments
    (re.compile(r"<[^>]+>"), "<sym>"),                                       # symbolic targets
    (re.compile(r"\b(s_(?:c)?branch\w*|s_call_b64)\s+.*$"), r"\1 <pc-rel>"),
]
# the literal of the s_add_u32 / s_addc_u32 pair that follows s_getpc_b64 directly (a pc-relative address), and of
# no other scalar add
PCREL_ADD = re.compile(r"\b(s_add_u32|s_addc_u32)\s+(s\d+), (s\d+), (0x[0-9a-f]+|-?\d+)\s*$")


def kernels(co):
    """{kernel symbol: [masked instruction lines]} of one code object."""
    names = set()
    for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", co], text=True).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
            names.add(f[7])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                   text=True)
    out, cur, after_getpc = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            after_getpc = 0
            if cur is not None:
                out[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        for rx, to in MASKS:
            line = rx.sub(to, line)
        line = line.strip()
        if after_getpc > 0:
            after_getpc = after_getpc - 1 if PCREL_ADD.search(line) else 0
            line = PCREL_ADD.sub(r"\1 \2, \3, <pc-rel>", line)
        if line.startswith("s_getpc_b64"):
            after_getpc = 2
        out[cur].append(line)
    for body in out.values():                # the padding up to the next symbol, or to the section's end
        while body and (body[-1] in ("s_nop 0", "...") or body[-1].startswith("s_code_end")):
            body.pop()
    return out


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        ko, kn = {}, {}
        for co in code_objects(old, tmp, "old"):
            ko.update(kernels(co))
        for co in code_objects(new, tmp, "new"):
            kn.update(kernels(co))
    both = sorted(set(ko) & set(kn))
    changed = [k for k in both if ko[k] != kn[k]]
    print(f"gfx950 kernels: {len(ko)} in the old build, {len(kn)} in the new one, {len(both)} in both")
    print("masked: addresses, branch targets, the literals of the s_add_u32 / s_addc_u32 pair directly behind an "
          "s_getpc_b64 (no other scalar add); compared instruction by instruction, trailing alignment padding dropped\n")
    for k in both:
        print(f"{'DIFFERS' if k in changed else 'same   '} {len(kn[k]):6d} instructions  {k}")
    print("\nonly in the new build:")
    for k in sorted(set(kn) - set(ko)):
        print(f"        {len(kn[k]):6d} instructions  {k}")
    print("\nonly in the old build:")
    for k in sorted(set(ko) - set(kn)):
        print(f"        {len(ko[k]):6d} instructions  {k}")
    print(f"\nverdict: {len(changed)} of {len(both)} kernels that exist in both builds changed" +
          (" -- no existing kernel changed" if not changed else ""))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
