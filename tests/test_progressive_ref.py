"""The Python restatement of progressive decoding (tests/progressive_ref.py) against the CPU oracle and Pillow: its
decoder on Pillow's pinned files, its encoder through Pillow. Needs Pillow."""
import io

import numpy as np
import pytest

from tests import progressive_cases as pc
from tests import progressive_ref as pr

Image = pytest.importorskip("PIL.Image")


def test_decoder_on_the_pins_equals_the_oracle_on_the_twins():
    from oracle import oracle

    for name, (prog, twin, _) in pc.pins().items():
        d, o = pr.decode(prog), oracle.decode(twin)
        assert len(d.coef) == o.ncomp, name
        for c, (vy, vx) in enumerate(d.visible):
            assert np.array_equal(d.coef[c][:vy, :vx], o.coef[c][:vy, :vx]), (name, c)
    scans = {name: len(pr.decode(prog).scans) for name, (prog, _, _) in pc.pins().items()}
    assert scans["pgray"] == 6 and scans["p420"] == 10 and scans["pcmyk"] == 18
    assert max(s["segments"] for s in pr.decode(pc.pins()["p420_rst1"][0]).scans) == 153


def test_pillow_opens_what_the_encoder_writes():
    """Every complete script: Pillow returns the pixels of the baseline original (three components and grey; Pillow takes a
    four-component file without an Adobe segment for CMYK, as it does the original)."""
    for name in pc.COMPLETE:
        prog, base = pc.crafted()[name]
        a = np.asarray(Image.open(io.BytesIO(prog)).convert("RGB"))
        b = np.asarray(Image.open(io.BytesIO(base)).convert("RGB"))
        assert np.array_equal(a, b), name


def test_decoder_reads_back_what_the_encoder_was_given():
    from oracle import oracle

    for name in pc.COMPLETE:
        prog, base = pc.crafted()[name]
        d, o = pr.decode(prog), oracle.decode(base)
        for c, (vy, vx) in enumerate(d.visible):
            assert np.array_equal(d.coef[c][:vy, :vx], o.coef[c][:vy, :vx]), (name, c)
