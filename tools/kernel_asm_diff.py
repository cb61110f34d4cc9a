"""Did a source change move the device code?  Compiles one translation unit at a git revision and in the working tree
(build.py's FLAGS + --cuda-device-only -S) and compares the assembly, whole and per kernel:
    python tools/kernel_asm_diff.py [--map OLD=NEW]... REV SOURCE.hip [extra hipcc flags]
--map: a kernel whose mangled name changed on purpose (a template parameter gone) - OLD is replaced by NEW in REV's text.
Comment lines, .file / .loc / .ident and the __hip_cuid_ lines (they carry paths and hashes of paths) are dropped.  Per
kernel symbol: its instruction lines, how many differ once the function index of the local labels is masked, and whether
the .amdhsa_ descriptor lines are equal.  Exit status 0: nothing differs.  CPU only; reads nothing but compiler output."""
import difflib
import importlib.util
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DROP = re.compile(r"\s*(;|//|\.file\b|\.loc\b|\.ident\b)|.*__hip_cuid_")
_LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")


def normalise(text):
    """The lines of an assembly text that a source move cannot excuse: no comment lines, no .file / .loc / .ident,
    no __hip_cuid_ lines, no trailing blanks, no empty lines."""
    return [ln.rstrip() for ln in text.splitlines() if ln.strip() and not _DROP.match(ln)]


def mask_labels(line):
    """.LBB12_3 -> .LBB#_3, .Lfunc_end12 -> .Lfunc_end#: the index counts the functions in front of this one."""
    return _LABEL.sub(lambda m: ".L" + m.group(1) + "#", line)


def kernels(lines):
    """{kernel symbol: (instruction lines with labels masked, .amdhsa_ descriptor lines)} of normalised lines.  A kernel
    is a symbol with an .amdhsa_kernel block; its instructions run from its label to its .Lfunc_end."""
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.split(";")[0].strip() == name + ":")
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[start + 1:end]
        desc = [ln.strip() for ln in body if ln.strip().startswith(".amdhsa_") and not ln.strip().startswith(".amdhsa_kernel")]
        # (a label's trailing comment names its loop header with the unmasked function index: "; in Loop: Header=BB16_40")
        insns = [mask_labels(ln.split(";")[0].strip()) for ln in body if not ln.strip().startswith(".") or ln.strip().startswith(".LBB")]
        out[name] = (insns, desc)
    return out


def compare(old_text, new_text):
    """(whole text equal, [(kernel, instruction lines old, new, differing lines, descriptor equal)]); a kernel that one
    side lacks has None for that side's count."""
    old, new = normalise(old_text), normalise(new_text)
    ko, kn = kernels(old), kernels(new)
    rows = []
    for name in list(ko) + [n for n in kn if n not in ko]:
        io_, do_ = ko.get(name, (None, None))
        in_, dn_ = kn.get(name, (None, None))
        if io_ is None or in_ is None:
            rows.append((name, io_ and len(io_), in_ and len(in_), len(io_ or in_), False))
            continue
        differing = sum(1 for d in difflib.ndiff(io_, in_) if d[0] in "+-") if io_ != in_ else 0
        rows.append((name, len(io_), len(in_), differing, do_ == dn_))
    return old == new, rows


def _flags():
    spec = importlib.util.spec_from_file_location("_coevo_build", os.path.join(REPO, "coevonet_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FLAGS


def _assembly(root, source, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + _flags() + extra + ["--cuda-device-only", "-S", os.path.join(root, "coevonet_amd", "csrc", source), "-o", "-"]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def main(argv):
    renames = []
    while len(argv) > 1 and argv[0] == "--map":
        renames.append(argv[1].split("=", 1))
        argv = argv[2:]
    if len(argv) < 2:
        sys.exit(__doc__)
    rev, source, extra = argv[0], argv[1], argv[2:]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", REPO, "archive", rev, "coevonet_amd/csrc", "include"], check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        with ThreadPoolExecutor(2) as ex:
            old, new = ex.map(lambda root: _assembly(root, source, extra), (tmp, REPO))
    for a, b in renames:
        old = old.replace(a, b)
    same, rows = compare(old, new)
    demangled = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    ok = same
    for (name, n_old, n_new, differing, desc_same), dn in zip(rows, demangled):
        dn = re.sub(r"\(.*", "", dn)
        if n_old is None or n_new is None:
            print(f"{dn:70s} only at {rev if n_new is None else 'the working tree'} ({differing} instruction lines)")
            ok = False
            continue
        print(f"{dn:70s} {n_new:6d} instruction lines  {differing:5d} differ  descriptor {'equal' if desc_same else 'DIFFERS'}")
        ok = ok and differing == 0 and desc_same and n_old == n_new
    print(f"{source} {' '.join(extra)}: {len([r for r in rows if r[2] is not None])} kernels in the working tree, "
          f"{len([r for r in rows if r[1] is not None])} at {rev}; whole text {'equal' if same else 'DIFFERS'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
