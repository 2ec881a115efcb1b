"""Mutation fuzzing of progressive decoding on the host under AddressSanitizer + UBSan: the product's parser, the scan
bodies of jg_prog_core.h (through the host twin, tests/emu/prog_twin.cpp) and the hand-over's pack, on mutated copies of
Pillow's pinned progressive files, of the two files of long end-of-band runs and of one with a padded work list. A
stand-alone program (tests/emu/prog_fuzz_main.cpp): corrupt streams are exercised here only, never on the GPU, whose
kernels compile the same jg_prog_core.h."""
import os
import subprocess
import sys
import tempfile

import pytest

from tests import progressive_cases as pc
from tests.emu import prog_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_mutated_progressive_streams_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "prog_fuzz_main")
        srcs = [os.path.join(ROOT, "tests", "emu", "prog_fuzz_main.cpp")] + prog_twin.sources()
        subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                              + prog_twin.compile_args() + srcs + ["-o", exe])
        files = []
        inputs = {name: prog for name, (prog, _, _) in pc.pins().items()}
        # end-of-band runs of every category and of 0x7FFF blocks (mutated, they meet the clamp of a run to the blocks
        # left in the segment), and a work list with idle items
        inputs.update({name: pc.large()[name].prog for name in ("eob_ladder", "eob_cap")})
        inputs["two_large_444"] = pc.structure()["two_large_444"][0]
        assert len(inputs) == 10 + 3
        for name, prog in sorted(inputs.items()):
            p = os.path.join(d, name + ".jpg")
            with open(p, "wb") as f:
                f.write(prog)
            files.append(p)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, "1500", "20261017"] + files, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
        sys.stdout.write(r.stdout.decode())
        assert r.returncode == 0, r.stderr.decode()[-4000:]
        out = r.stdout.decode()
        assert "decoded" in out
        decoded = int(out.split(" iterations, ")[1].split(" decoded")[0])
        # a fifth of the mutations damage entropy-coded bytes only and keep the file's structure: those all reach the scan bodies
        assert decoded >= 300, "too few mutations get past the parser to exercise the scan bodies: " + out
