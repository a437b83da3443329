"""Compare the gfx950 instruction streams of two source trees, kernel by kernel.

    python tools/isa_identity.py emit <tree> <outdir>       # compile every .hip of _build.SOURCES to <outdir>/<file>.s
    python tools/isa_identity.py compare <dirA> <dirB> [--allow REGEX] [--kernarg]

emit uses the tree's own _build.FLAGS / FILE_FLAGS plus --offload-device-only -S.  compare splits each .s at the kernel
symbols (`_Z...:` to `.Lfunc_end`), drops comments and normalises the function-numbered local labels, then reports the
symbol sets and every kernel whose body differs.  Exit status 1 if a kernel outside --allow differs or a symbol of A is missing in B or
a symbol outside --allow is new in B.
--kernarg: a field appended to a struct that kernels take BY VALUE (falnet_conv_t) moves every argument behind it and the hidden arguments:
the kernel-argument loads change their offsets and nothing else.  With this switch the scalar instructions that carry such an offset
(s_load_*, s_add_u32 / s_addc_u32, s_mul*) and the .amdhsa_kernarg_size directive are compared with their numbers masked; every other line
(all vector, MFMA, LDS and memory instructions, all branches) still has to match exactly, and the count of masked-only kernels is reported.
"""
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def emit(tree, out):
    spec = importlib.util.spec_from_file_location("_b", os.path.join(tree, "fal_net_amd", "_build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(out, exist_ok=True)
    srcs = [s for s in b.SOURCES if s.endswith(".hip")]
    # largest first: conv.hip dominates the wall time
    srcs.sort(key=lambda s: -os.path.getsize(os.path.join(b.CSRC, s)))

    def run(s):
        cmd = [b.HIPCC] + b.FLAGS + b.FILE_FLAGS.get(s, []) + ["--offload-device-only", "-S", "-x", "hip", os.path.join(b.CSRC, s), "-o", os.path.join(out, s + ".s")]
        subprocess.run(cmd, check=True)
        print("done", s, flush=True)
    with ThreadPoolExecutor(max_workers=int(os.environ.get("JOBS", "4"))) as ex:
        list(ex.map(run, srcs))


_LABEL = re.compile(r"\.(LBB|LJTI|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def kernels(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if not f.endswith(".s"):
            continue
        name, body = None, []
        for line in open(os.path.join(d, f)):
            line = line.split(";")[0].rstrip()
            if not line.strip():
                continue
            m = re.match(r"^(_Z\w+):$", line)
            if m and name is None:
                name, body = m.group(1), []
                continue
            if name is not None:
                if line.startswith(".Lfunc_end"):
                    out[name] = "\n".join(body)
                    name = None
                else:
                    body.append(_LABEL.sub(lambda k: "." + k.group(1) + "N", line))
    return out


_KERNARG_LINE = re.compile(r"^\s*(s_load_dword\w*|s_add_u32|s_addc_u32|s_mul\w*|\.amdhsa_kernarg_size)\b")
_NUMBER = re.compile(r"0x[0-9a-f]+|\b\d+\b")


def mask_kernarg(body):
    return "\n".join(_NUMBER.sub("N", line) if _KERNARG_LINE.match(line) else line for line in body.split("\n"))


def compare(a, b, allow, kernarg=False):
    ka, kb = kernels(a), kernels(b)
    if kernarg:
        exact = sum(1 for s in set(ka) & set(kb) if ka[s] == kb[s])
        ka, kb = {s: mask_kernarg(v) for s, v in ka.items()}, {s: mask_kernarg(v) for s, v in kb.items()}
        same = sum(1 for s in set(ka) & set(kb) if ka[s] == kb[s])
        print(f"--kernarg: {exact} bodies identical as they are, {same - exact} more once the kernel-argument offsets are masked")
    print(f"kernel symbols: {len(ka)} in {a}, {len(kb)} in {b}")
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    for s in only_a:
        print("only in A:", s)
    for s in only_b:
        print("only in B:", s)
    diff = sorted(s for s in set(ka) & set(kb) if ka[s] != kb[s])
    bad = [s for s in diff if not (allow and re.search(allow, s))]
    print(f"identical bodies: {len(set(ka) & set(kb)) - len(diff)}; differing: {len(diff)} ({len(diff) - len(bad)} permitted)")
    for s in diff:
        print("  differs%s: %s" % ("" if s in bad else " (permitted)", s))
    return 1 if (bad or only_a or [s for s in only_b if not (allow and re.search(allow, s))]) else 0


if __name__ == "__main__":
    if sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3])
    else:
        allow = sys.argv[sys.argv.index("--allow") + 1] if "--allow" in sys.argv else None
        sys.exit(compare(sys.argv[2], sys.argv[3], allow, "--kernarg" in sys.argv))
