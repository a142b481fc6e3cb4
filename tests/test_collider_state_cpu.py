"""The solids' modes (pbf-sph_amd/csrc/pbf_collider_state.hpp): which of lattice / scenery / pose / reaction / body / friction is
on, what the step's reaction records describe, and the events that move either.  host/test_collider_state.cpp walks the struct
through the call sequences the entry points and the step perform and checks the header's rules after every event — no device,
not linked against the library; its _san twin is the same program under the address and undefined-behaviour sanitizers.  And
the rule that makes that walk meaningful: pbf_hip.hip changes the modes through the events only, never by assigning to a field,
and keeps no copy of a flag beside the struct.  The two lattices (csrc/pbf_solid_lattice.hpp) are held to the same: one record,
one function that builds kernel arguments from it, one install path, and no field assigned outside the header."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "pbf-sph_amd"
STATE = (PKG / "csrc" / "pbf_collider_state.hpp").read_text()
LATTICE = (PKG / "csrc" / "pbf_solid_lattice.hpp").read_text()
SRC = (PKG / "csrc" / "pbf_hip.hip").read_text()

FIELDS = re.findall(r"^  (?:bool|int|uint64_t) (\w+) = [-\w]+;", STATE, re.M)
OLD_NAMES = ["colliderPosed", "reactionOn", "bodyOn", "frictionOn", "frictionRan", "pushAt", "pushRows", "colliderGen",
             "colliderPhi", "colliderDims", "colliderOrigin", "colliderSpacing", "colliderMargin", "collider_args", "scenery_args",
             "collider_install", "scenery_install", "pair_needs_reaction", "SceneryState"]
ASSIGNMENT = r"[^\n]*\bcol\s*\.\s*\w+\s*(?:[-+*/|&^]|<<|>>)?=(?!=)[^\n]*"
# a SolidLattice is reached as `ctx->solid[which]`, or through a reference to one (`l` in pbf_hip.hip)
LATTICE_FIELDS = ["phi", "dims", "origin", "spacing", "margin"]
LATTICE_ASSIGNMENT = (r"[^\n]*(?:\bsolid\s*\[[^\]\n]*\]|\bl)\s*\.\s*(?:%s)\b\s*(?:\.\s*\w+\s*)?(?:\[[^\]\n]*\]\s*)?"
                      r"(?:[-+*/|&^]|<<|>>)?=(?!=)[^\n]*" % "|".join(LATTICE_FIELDS))
STEPPED = r"[^\n]*(?:\+\+|--)\s*\w+(?:->|\.)col\s*\.\s*\w+[^\n]*|[^\n]*\bcol\s*\.\s*\w+\s*(?:\+\+|--)[^\n]*"


@pytest.mark.parametrize("program", ["test_collider_state", "test_collider_state_san"])
def test_state_machine_walk(pkg, program):
    r = subprocess.run([str(PKG / program)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "collider state ok" in r.stdout and "18 flag combinations reached" in r.stdout, r.stdout


def test_the_header_declares_the_fields_this_test_knows():
    assert set(FIELDS) == {"lattice", "scenery", "posed", "reaction", "body", "friction", "frictionRan", "gen", "pushAt", "pushRows"}
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


def test_one_lattice_record_one_argument_builder_one_install_path():
    code = re.sub(r"//[^\n]*", "", SRC)
    assert "#include <hip" not in LATTICE and "__device__" not in LATTICE and "__global__" not in LATTICE and "hip_runtime" not in LATTICE
    assert len(re.findall(r"^template <typename Buf> struct SolidLattice \{", LATTICE, re.M)) == 1
    members = re.sub(r"//[^\n]*", "", re.search(r"  Buf phi;.*?margin = 0;", LATTICE, re.S).group(0))
    assert set(LATTICE_FIELDS) == set(re.findall(r"\b([a-z]\w*)(?=\[3\]| = |;)", members))
    assert len(re.findall(r"^int solid_install\(", code, re.M)) == 1
    assert len(re.findall(r"^template <typename N> ColliderSdf<N> sdf_args\(const SolidLattice<DevBuf> &", code, re.M)) == 1
    # pbf_ctx holds the two as one indexed pair, and no other object of the type exists
    assert len(re.findall(r"\bSolidLattice<DevBuf> solid\[2\];", code)) == 1 and len(re.findall(r"\bSolidLattice<DevBuf> \w", code)) == 1
    # no field of either lattice is assigned outside the header: put() is the one mutator, and solid_install alone calls it
    hits = re.findall(LATTICE_ASSIGNMENT, code)
    assert not hits, hits
    assert not re.search(r"\bsolid\s*\[[^\]\n]*\]\s*=(?!=)", code)
    assert len(re.findall(r"\.put\(", code)) == 1
    install = re.search(r"^int solid_install\(.*?\n\}", code, re.S | re.M).group(0)
    assert ".put(" in install and install.index("collider_drop_graphs(ctx)") < install.index(".put(")
    # the captured steps' key has one generation for both solids
    key = re.search(r"struct GraphKey \{(.*?)\n\};", code, re.S).group(1)
    assert re.search(r"\buint64_t collider;", key) and "scenery" not in key, key
    assert not re.search(r"\bk\.scenery\b", code)


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
    for bad in ["ctx->solid[which].phi = std::move(fresh);", "ctx->solid[0].dims[a] = sdf->dims[a];", "  ctx->solid [1] . margin=0;",
                "c.solid[ColliderState::SCENERY].spacing *= 2;", "l.origin[a] = 0.0;", "ctx->solid[which].phi.p = nullptr;",
                "for (;;) ctx->solid[1].dims[a] = 0u, ctx->solid[1].origin[a] = 0.0;"]:
        assert re.findall(LATTICE_ASSIGNMENT, bad), bad
    for ok in ["s.phi = ctx->solid[0].phi.as<const N>();", "s.dims[a] = l.dims[a], s.origin[a] = N(l.origin[a]);",
               "s.inv = N(1) / N(l.spacing), s.margin = N(l.margin);", "if (ctx->solid[1].spacing == 0) f();",
               "ctx->solid[which].put(sdf, fresh);", "a(ctx->solid[0].dims[0] >= 2)", "k.collider = ctx->col.gen;"]:
        assert not re.findall(LATTICE_ASSIGNMENT, ok), ok
