"""What jpeggpu_amd's batched wrappers refuse before they touch a device or an ImgInfo -- the one resize call path behind
resize_scratch_size, resize_to_rgb, resize_to_tensor and resize_views_to_tensor, and batch_to_rgb -- and the symbols a
library loaded through JPEGGPU_LIB may predate. No GPU: the planes are dummy CPU tensors and every info is None, so a check
that came too late would fail with something other than the ValueError asked for."""
import pytest

import jpeggpu_amd
from jpeggpu_amd import api

VIEW = (8, 8, 0, 0)
# wrapper -> (the positional arguments behind planes_list and infos, its per-image lists besides infos, what else it checks)
WRAPPERS = {
    "resize_scratch_size": ((8,), ("crop_infos", "colors", "orientations"), ("filt",)),
    "resize_to_rgb": ((8,), ("crop_infos", "colors", "orientations"), ("filt", "layout")),
    "resize_to_tensor": ((8,), ("crop_infos", "colors", "orientations", "flips"), ("filt", "layout", "dtype")),
    "resize_views_to_tensor": (([VIEW], 8), ("crop_infos", "colors", "orientations", "replicates", "flips"), ("filt", "layout", "dtype")),
    "batch_to_rgb": ((), ("crop_infos", "colors", "orientations", "replicates"), ("layout",)),
}


def planes_list():
    import torch

    return [[torch.zeros(1, dtype=torch.uint8)]]


@pytest.mark.parametrize("name", WRAPPERS)
def test_unknown_filter_layout_and_dtype(name):
    import torch

    fn, (args, _, checked) = getattr(jpeggpu_amd, name), WRAPPERS[name]
    bad = {"filt": "lanczos", "layout": "NWHC", "dtype": torch.float64}
    word = {"filt": "filter", "layout": "layout", "dtype": "dtype"}
    for key in checked:
        with pytest.raises(ValueError, match=word[key]):
            fn(planes_list(), [None], *args, **{key: bad[key]})
    # in the order filter, layout, dtype: the first one wrong is the one named
    for first, rest in (("filt", ("layout", "dtype")), ("layout", ("dtype",))):
        wrong = {k: bad[k] for k in (first,) + rest if k in checked}
        if first in wrong and len(wrong) > 1:
            with pytest.raises(ValueError, match=word[first]):
                fn(planes_list(), [None], *args, **wrong)


@pytest.mark.parametrize("name", WRAPPERS)
def test_per_image_lists_of_the_wrong_length(name):
    fn, (args, lists, _) = getattr(jpeggpu_amd, name), WRAPPERS[name]
    for wrong in ([], [None, None]):  # one image: too short, too long
        with pytest.raises(ValueError, match="infos must have one entry per image"):
            fn(planes_list(), wrong, *args)
        for key in lists:
            with pytest.raises(ValueError, match="%s must have one entry per image" % key):
                fn(planes_list(), [None], *args, **{key: wrong})
    if name == "resize_views_to_tensor":
        for wrong in ([], [VIEW, VIEW]):
            with pytest.raises(ValueError, match="views must have one entry per image"):
                fn(planes_list(), [None], wrong, 8)


def test_symbols_an_older_library_lacks(monkeypatch):
    """Batch.set_fused_tail, Batch.set_sync_run and fused_tail_timeouts name the symbol the loaded library does not have."""
    class Older:
        pass

    monkeypatch.setattr(api, "lib", lambda: Older())
    batch = object.__new__(jpeggpu_amd.Batch)  # (no jpeggpu_ext_batch_create: the check comes before the handle is used)
    batch._h = None
    with pytest.raises(RuntimeError, match="jpeggpu_ext_batch_set_fused_tail"):
        batch.set_fused_tail(True)
    with pytest.raises(RuntimeError, match="jpeggpu_ext_batch_set_sync_run"):
        batch.set_sync_run(2)
    with pytest.raises(RuntimeError, match="jpeggpu_ext_fused_tail_timeouts"):
        jpeggpu_amd.fused_tail_timeouts()
