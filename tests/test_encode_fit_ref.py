"""The rule of jpeggpu_ext_encode_fit_batch restated (tests/encode_fit_ref.py) against Pillow's pinned tables and files
(tests/golden/encode_fit_pins.npz, tools/make_encode_fit_pins.py), and what the case list must hold. No GPU needed."""
import hashlib

from tests import encode_fit_ref as F

CASES = F.cases()
PINS = F.pins()[0]
MIN_DIFFERENT = 5


def test_case_list_covers_what_it_must():
    assert len(CASES) >= 40 and len({c["name"] for c in CASES}) == len(CASES) and {c["name"] for c in CASES} == set(PINS)
    assert {(c["w"], c["h"]) for c in CASES} == set(F.SIZES)
    for key, values in (("grey", (False, True)), ("subsampling", F.SUBSAMPLINGS), ("restart_interval", F.INTERVALS), ("optimize", (False, True))):
        assert {c[key] for c in CASES} == set(values), key
    widths = {c["hi"] - c["lo"] + 1 for c in CASES}
    assert {1, 2, 100} <= widths
    # both kinds of table under every subsampling, and grey with either
    assert {(c["optimize"], c["subsampling"]) for c in CASES if not c["grey"]} == {(o, s) for o in (False, True) for s in F.SUBSAMPLINGS}
    assert {c["optimize"] for c in CASES if c["grey"]} == {False, True}


def test_pillow_sizes_are_not_monotone_and_the_rule_is_not_the_largest_fitting_quality():
    """At least five cases hold a budget in a dip of Pillow's own table for which bisection and `the largest quality that
    fits` part: the pins can tell the two apart."""
    different = []
    for c in CASES:
        table = PINS[c["name"]]["table"]
        for e in PINS[c["name"]]["budgets"]:
            want = F.choose(table.__getitem__, c["lo"], c["hi"], e["budget"])
            assert (want if want is not None else -1) == e["quality"], (c["name"], e)
            if want != F.largest_fitting(table.__getitem__, c["lo"], c["hi"], e["budget"]):
                different.append(c["name"])
                assert want is not None and table[want] <= e["budget"], "the rule's file always fits"
    assert len(set(different)) >= MIN_DIFFERENT, sorted(set(different))
    example = PINS["fit_37x39_gradient_rgb_420_r0_std_q1_100_example"]["table"]
    assert F.dips(example, 1, 100), "the 37 x 39 gradient at 4:2:0 has a quality whose successor is smaller"


def test_pinned_budgets_are_the_ones_the_tests_derive():
    for c in CASES:
        table = PINS[c["name"]]["table"]
        assert [e["budget"] for e in PINS[c["name"]]["budgets"]] == F.budgets(table, c["lo"], c["hi"], 6), c["name"]
        kinds = {e["quality"] for e in PINS[c["name"]]["budgets"]}
        assert -1 in kinds and c["hi"] in kinds, c["name"]  # over budget, and the upper end


def test_the_rule_asks_for_no_more_sizes_than_the_host_plans():
    for lo, hi in [(1, 100), (1, 1), (7, 8), (1, 3), (1, 4), (1, 5), (10, 90), (1, 66), (1, 67), (34, 100)]:
        table = {q: q for q in range(1, 101)}  # a monotone table
        worst = 0
        for budget in range(0, 102):
            asked = []
            F.choose(lambda q: (asked.append(q), table[q])[1], lo, hi, budget)
            assert len(asked) == len(set(asked)) or lo == hi  # (one quality: the rule asks for it as hi and as lo)
            worst = max(worst, len(set(asked)))
        assert worst == F.evaluations(lo, hi), (lo, hi)
    assert F.evaluations(1, 100) == 9 and F.launches(1, 100, False) == 82 and F.launches(1, 100, True) == 102


def test_restatement_equals_the_pins():
    """Every size of the restated encoder over every case's range, and for every pinned budget the quality and the file."""
    for c in CASES:
        pin = PINS[c["name"]]
        img, files = F.image(c), {}

        def size(q):
            if q not in files:
                files[q] = F.encode(c, q, img)
            return len(files[q])

        step = 1 if c["w"] * c["h"] <= 1200 else 7  # the whole table of the small cases, a stride of the others
        for q in range(c["lo"], c["hi"] + 1, step):
            assert size(q) == pin["table"][q], (c["name"], q)
        for e in pin["budgets"]:
            q = F.choose(size, c["lo"], c["hi"], e["budget"])
            assert (q if q is not None else -1) == e["quality"], (c["name"], e)
            if q is None:
                assert size(c["lo"]) == e["length"] > e["budget"]
                continue
            assert F.equals_pin(c["name"], e, files[q]), (c["name"], e)
            assert len(files[q]) == e["length"] <= e["budget"] and hashlib.sha256(files[q]).hexdigest() == e["sha256"]
