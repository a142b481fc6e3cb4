"""The collider's modes (pbf-sph_amd/csrc/pbf_collider_state.hpp): which of lattice / pose / reaction / body / friction is on,
what the step's reaction records describe, and the events that move either.  host/test_collider_state.cpp walks the struct
through the call sequences the entry points and the step perform and checks the header's rules after every event — no device,
not linked against the library; its _san twin is the same program under the address and undefined-behaviour sanitizers.  And
the rule that makes that walk meaningful: pbf_hip.hip changes the modes through the events only, never by assigning to a field,
and keeps no copy of a flag beside the struct."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "pbf-sph_amd"
STATE = (PKG / "csrc" / "pbf_collider_state.hpp").read_text()
SRC = (PKG / "csrc" / "pbf_hip.hip").read_text()

FIELDS = re.findall(r"^  (?:bool|int|uint64_t) (\w+) = [-\w]+;", STATE, re.M)
OLD_NAMES = ["colliderPosed", "reactionOn", "bodyOn", "frictionOn", "frictionRan", "pushAt", "pushRows", "colliderGen"]
ASSIGNMENT = r"[^\n]*\bcol\s*\.\s*\w+\s*(?:[-+*/|&^]|<<|>>)?=(?!=)[^\n]*"
STEPPED = r"[^\n]*(?:\+\+|--)\s*\w+(?:->|\.)col\s*\.\s*\w+[^\n]*|[^\n]*\bcol\s*\.\s*\w+\s*(?:\+\+|--)[^\n]*"


@pytest.mark.parametrize("program", ["test_collider_state", "test_collider_state_san"])
def test_state_machine_walk(pkg, program):
    r = subprocess.run([str(PKG / program)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "collider state ok" in r.stdout and "10 flag combinations reached" in r.stdout, r.stdout


def test_the_header_declares_the_fields_this_test_knows():
    assert set(FIELDS) == {"lattice", "posed", "reaction", "body", "friction", "frictionRan", "gen", "pushAt", "pushRows"}
    assert "#include <hip" not in STATE and "__device__" not in STATE and "__global__" not in STATE and "hip_runtime" not in STATE


def test_no_field_of_the_modes_is_assigned_outside_the_header():
    code = re.sub(r"//[^\n]*", "", SRC)
    # the struct is reached as `ctx->col`; a whole-struct copy would be `ctx->col = ...` without a field, and there is none
    hits = re.findall(ASSIGNMENT, code) + re.findall(STEPPED, code)
    assert not hits, hits
    assert not re.search(r"(?:->|\.)col\s*=(?!=)", code)
    # no flag lives on in pbf_ctx beside the struct, and nothing takes a field's address to write through it
    for f in FIELDS:
        assert not re.search(r"ctx->%s\b" % f, code), f
        assert not re.search(r"(?<!&)&(?!&)\s*\w+(?:->|\.)col\s*\.\s*%s\b" % f, code), f
    assert len(re.findall(r"\bColliderState col;", code)) == 1
    # the captured steps' key takes the struct's generation, and dropping the graphs counts nothing itself
    assert re.search(r"k\.collider = ctx->col\.gen;", code)
    drop = re.search(r"int collider_drop_graphs\(pbf_ctx \*ctx\) \{(.*?)\n\}", code, re.S).group(1)
    assert "++" not in drop and "col." not in drop, drop


def test_none_of_the_old_names_remains():
    for name in OLD_NAMES:                                     # (comments included)
        assert not re.search(r"\b%s\b" % name, SRC), name
    # the slab refusal of the collider code is spelt once
    assert SRC.count("ctx->comm || ctx->slabActive || ctx->slabConfigured") == 1
    assert SRC.count("kColliderSlabError") == 3                # its definition, the helper, pbf_slab_configure / attach's own test


def test_the_regular_expression_sees_an_assignment():
    for bad in ["ctx->col.posed = false;", "  ctx->col.pushRows=rows;", "c->col . gen |= 1;", "x.col.gen += 1;",
                "ctx->col.pushAt = ctx->orderEpoch, ctx->col.pushRows = -1;"]:
        assert re.findall(ASSIGNMENT, bad), bad
    for bad in ["ctx->col.gen++;", "++ctx->col.gen;", "--c.col.pushRows;"]:
        assert re.findall(STEPPED, bad), bad
    for ok in ["if (ctx->col.reaction) return;", "ctx->col.installed(sdf != nullptr);", "k.collider = ctx->col.gen;",
               "const bool turnOn = !ctx->col.friction;", "a(ctx->col.posed != b)", "b(ctx->col.gen <= 1, x >= 2)",
               "return ctx->col.pose_set() ? collider_drop_graphs(ctx) : PBF_OK;", "if (ctx->col.pushRows == 1) f();"]:
        assert not re.findall(ASSIGNMENT, ok) and not re.findall(STEPPED, ok), ok
