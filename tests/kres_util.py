"""Compile one translation unit of csrc/ for gfx950 with the compiler's kernel-resource remarks and parse them: what
the kernel-resource tests assert on and what tools/kres.py prints.  hipcc cross-compiles without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "btl_bloomfilter_amd", "csrc")

# key -> the remark line that carries it (the SGPR line reads "TotalSGPRs:"; a plain "SGPRs:" is taken too)
_KEYS = (("sgpr", r" (?:Total)?SGPRs: (\d+)"), ("vgpr", r" VGPRs: (\d+)"), ("agpr", r" AGPRs: (\d+)"),
         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def short_name(mangled):
    """the demangled name without `void `, the namespace and the parameter list (cut at the parenthesis that matches the
    last one, so that a cast inside the template arguments, `<(Enum)1>`, stays part of the name)"""
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                name = name[:i]
                break
    return name.replace("void ", "").replace("btlbf::", "")


def parse_remarks(stderr):
    """{kernel name without namespace and arguments: {"sgpr", "vgpr", "agpr", "scratch", "lds"}} in the unit's order"""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(short_name(m.group(1)), {})
        elif cur is not None:
            for key, pat in _KEYS:
                m = re.search(pat, line)
                if m:
                    cur[key] = int(m.group(1))
    return out


def compile_remarks(unit, obj, flags=()):
    """(hipcc's return code, its stderr) of `unit` (a file name in csrc/) compiled to `obj` with the remarks on"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "hipcc is part of the image: the build check needs it too"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", *flags, "-c", "-o", str(obj), os.path.join(CSRC, unit)],
                       capture_output=True, text=True)
    return r.returncode, r.stderr


def kernel_resources(unit, obj, flags=()):
    rc, err = compile_remarks(unit, obj, flags)
    assert rc == 0, err[-3000:]
    return parse_remarks(err)
