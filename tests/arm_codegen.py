"""wbc_arm_kernel.hip compiled to gfx950 assembly with the build's own flags, for the *_codegen tests of the kernels in it: one compile per
process, whichever tests ask."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCE = "wbc_arm_kernel.hip"


@functools.lru_cache(maxsize=None)
def _compiled():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    flags = [f for f in g.COMMON_FLAGS if f != "-fPIC"] + g.EXTRA_FLAGS.get(SOURCE, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "arm.s")
        subprocess.check_call([HIPCC] + flags + ["-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-o", out,
                               os.path.join(ROOT, "deep-whole-body-control_amd", "csrc", SOURCE)], stderr=subprocess.DEVNULL)
        text = open(out).read()
    return text, text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")


def assembly():
    """The whole file's assembly text (skips the calling test where there is no hipcc)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _compiled()[0]


def meta(kernel, key):
    """Integer field `key` (e.g. "private_segment_fixed_size") of the kernel's entry in the code object's metadata."""
    assembly()
    entry = next(e for e in _compiled()[1] if re.search(r"\.name:\s+%s\n" % kernel, e))
    return int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))


def body(kernel, end=".Lfunc_end"):
    """The kernel's instructions, from its label up to `end`: by default the whole function, out-of-line blocks included."""
    text = assembly()
    text = text[text.index("\n%s:" % kernel):]
    return text[:text.index(end)]
