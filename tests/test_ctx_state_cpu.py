"""The context's derived state (pbf-sph_amd/csrc/pbf_state.hpp): which buffer holds the truth, and the events that move it.
host/test_state.cpp walks the struct through the event sequences the library performs and checks the invariants after
every event — no device, not linked against the library.  And the rule that makes that walk meaningful: pbf_hip.hip changes
the state through the events only, never by assigning to a field."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "pbf-sph_amd"
STATE = (PKG / "csrc" / "pbf_state.hpp").read_text()
SRC = (PKG / "csrc" / "pbf_hip.hip").read_text()

FIELDS = re.findall(r"^  (?:bool|int|uint32_t) (\w+) = \w+;", STATE, re.M)


def test_state_machine_walk(pkg):
    r = subprocess.run([str(PKG / "test_state")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "state ok" in r.stdout


def test_the_header_declares_the_flags_this_test_knows():
    assert set(FIELDS) == {"cur", "pcur", "rcur", "countedTableN", "sorted", "counted", "bricksValid", "rowColValid",
                           "rowsValid", "rowsCurrent", "pstarInRows", "nbrValid", "nbrRows", "qposValid", "omegaValid",
                           "surfaceValid", "prePredicted"}
    assert "#include <hip" not in STATE and "__device__" not in STATE


def test_no_field_of_the_state_is_assigned_outside_its_header():
    code = re.sub(r"//[^\n]*", "", SRC)
    # the state is reached as `ctx->st` (or `<expr>.st` of a StepState copy); whole-struct copies (snapshot / restore) are
    # `st = ...` without a field and are allowed
    hits = re.findall(r"[^\n]*\bst\s*\.\s*\w+\s*(?:[-+*/|&^]|<<|>>)?=(?!=)[^\n]*", code)
    hits += re.findall(r"[^\n]*(?:\+\+|--)\s*\w+(?:->|\.)st\s*\.\s*\w+[^\n]*|[^\n]*\bst\s*\.\s*\w+\s*(?:\+\+|--)[^\n]*", code)
    assert not hits, hits
    # none of the flags lives on in pbf_ctx beside the struct, and nothing takes a field's address to write through it
    for f in FIELDS:
        assert not re.search(r"ctx->%s\b" % f, code), f
        assert not re.search(r"(?<!&)&(?!&)\s*\w+(?:->|\.)st\s*\.\s*%s\b" % f, code), f
    assert re.search(r"\bDerivedState st;", code)


def test_the_regular_expression_sees_an_assignment():
    for bad in ["ctx->st.sorted = false;", "  ctx->st.pcur=s;", "c->st . rcur |= 1;", "x.st.cur += 1;"]:
        assert re.findall(r"[^\n]*\bst\s*\.\s*\w+\s*(?:[-+*/|&^]|<<|>>)?=(?!=)[^\n]*", bad), bad
    for ok in ["if (ctx->st.cur == 1) return;", "ctx->st = s.st;", "ctx->st.predicted(c.tableN, false);",
               "const int s = ctx->st.cur, d = 1 - s;", "a(ctx->st.pcur != s)", "b(ctx->st.rcur <= 1, x >= 2)"]:
        assert not re.findall(r"[^\n]*\bst\s*\.\s*\w+\s*(?:[-+*/|&^]|<<|>>)?=(?!=)[^\n]*", ok), ok
