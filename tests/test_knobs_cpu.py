"""CPU tests of how the library reads its environment switches (csrc/knobs.hpp): the parsing rule the test helpers restate is
the one the library follows, no source file beside knobs.hpp reads the environment, every switch the library names is in the
table of DESIGN section 7, and the retired switches are gone from the code and the documents.  No GPU compute call is made."""
import glob
import os
import re

import pytest

from tests.helpers.hierarchy import _atol
from tests.helpers.product import ROOT, ensure_built

pkg = ensure_built()

CSRC = os.path.join(ROOT, "fem-shell_amd", "csrc")
SCRATCH = "FEMSHELL_TEST_SCRATCH_KNOB"  # (no switch of the library: only this file reads it)
TEXTS = [None, "", "0", "1", "-3", "+7", " 12", "12abc", "abc", "1e3", "0x10"]  # None: not set
RETIRED = ["FEMSHELL_ASM_WAVES", "FEMSHELL_AMG_DENSE_SYMMETRIZE", "FEMSHELL_AMG_K_MASK", "FEMSHELL_AMG_POST_INCREMENT"]


def csrc_files():
    files = sorted(f for ext in ("cpp", "hip", "hpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) >= 40 and os.path.join(CSRC, "knobs.hpp") in files
    return files


@pytest.mark.parametrize("text", TEXTS)
def test_numbers_and_switches_follow_the_restated_rule(monkeypatch, text):
    """femshell_knob_long is tests/helpers/hierarchy.py::_atol (unset: the default; text that is no number: 0), and
    femshell_knob_flag is "unset: the default, set: that number is not 0" -- so =0 switches a default-on switch off and
    anything that parses to another number switches a default-off one on."""
    if text is None:
        monkeypatch.delenv(SCRATCH, raising=False)
    else:
        monkeypatch.setenv(SCRATCH, text)
    for default in (0, 5000):
        assert pkg.knob_long(SCRATCH, default) == _atol(SCRATCH, default), (text, default)
    for default in (0, 1):
        expected = bool(default) if text is None else _atol(SCRATCH, default) != 0
        assert pkg.knob_flag(SCRATCH, default) is expected, (text, default)


def test_the_restated_rule_on_the_cases_that_tell_rules_apart(monkeypatch):
    """(holds the restatement itself to plain figures, so that the comparison above cannot pass on a shared mistake)"""
    want = {"": 0, "0": 0, "1": 1, "-3": -3, "+7": 7, " 12": 12, "12abc": 12, "abc": 0, "1e3": 1, "0x10": 0}
    for text, value in want.items():
        monkeypatch.setenv(SCRATCH, text)
        assert _atol(SCRATCH, 5000) == value, text
    monkeypatch.delenv(SCRATCH)
    assert _atol(SCRATCH, 5000) == 5000


def test_only_knobs_hpp_reads_the_environment():
    for f in csrc_files():
        if os.path.basename(f) == "knobs.hpp":
            assert re.search(r"\bgetenv\b", open(f).read()), "knobs.hpp no longer reads the environment?"
        else:
            assert not re.search(r"getenv", open(f).read()), os.path.relpath(f, ROOT)


def design_table_names():
    """The names in the first column of the table of environment variables in DESIGN section 7."""
    names, inside = set(), False
    for line in open(os.path.join(ROOT, "DESIGN.md")):
        if line.startswith("| Variable | Default | Meaning |"):
            inside = True
        elif inside and not line.startswith("|"):
            break
        elif inside:
            names |= set(re.findall(r"FEMSHELL_[A-Z0-9_]+", line.split("|")[1]))
    return names


def test_every_switch_the_library_names_is_documented():
    documented = design_table_names()
    assert len(documented) >= 70
    for f in csrc_files():
        for lineno, line in enumerate(open(f), 1):
            for literal in re.findall(r'"((?:[^"\\]|\\.)*)"', line):
                for name in re.findall(r"FEMSHELL_[A-Z0-9_]+", literal):
                    assert name in documented, "%s:%d names %s, which DESIGN section 7 does not list" % (os.path.relpath(f, ROOT), lineno, name)


def test_the_retired_switches_are_gone():
    files = csrc_files() + [os.path.join(ROOT, d) for d in ("DESIGN.md", "README.md", "INTEGRATION.md")]
    for f in files:
        text = open(f).read()
        for name in RETIRED:
            assert name not in text, (os.path.relpath(f, ROOT), name)
