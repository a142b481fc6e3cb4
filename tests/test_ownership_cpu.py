"""Who frees what in pbf-sph_amd/csrc/pbf_hip.hip, read off its text (no device): device memory is freed by DevBuf alone and
pinned host memory by the pinned owner alone, so that a buffer added to pbf_ctx cannot be forgotten by pbf_destroy — which
therefore names no buffer at all."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = (ROOT / "pbf-sph_amd" / "csrc" / "pbf_hip.hip").read_text()
CODE = re.sub(r"//[^\n]*", "", SRC)

MEMBER_ADDRESS = r"(?<!&)&\s*ctx\s*->"     # (the address of a member, not `a && ctx->b`)
DEVICE_FREE = r"\bhipFree\s*\("
PINNED_CALL = r"\bhipHost(?:Malloc|Free)\s*\("
DELETED_COPY = r"\bDevBuf\s*\(\s*const\s+DevBuf\s*&\s*\w*\s*\)\s*=\s*delete\s*;"
DEFINITION = r"^(?=[A-Za-z_])(?:template\s*<[^>\n]*>\s*)?(?:struct\s+(\w+)[^;{\n]*|[\w:<>*& ]+?[ *&](\w+)\s*\([^;{}]*\)\s*(?:const\s*)?)\{"


def body(code, start):
    """the text between the brace that opens at or after `start` and its partner"""
    i = code.index("{", start)
    depth = 0
    for j in range(i, len(code)):
        depth += (code[j] == "{") - (code[j] == "}")
        if depth == 0:
            return code[i + 1:j]
    raise AssertionError("unbalanced braces")


def enclosing(code, pattern):
    """names of the top-level (column 0) struct or function definitions in which `pattern` occurs; a hit outside all of
    them counts as ''"""
    spans = []
    for m in re.finditer(DEFINITION, code, re.M):
        inner = body(code, m.end() - 1)
        spans.append((m.end(), m.end() + len(inner), m.group(1) or m.group(2)))
    names = []
    for hit in re.finditer(pattern, code):
        names.append(next((name for a, b, name in spans if a <= hit.start() < b), ""))
    return names


def test_destroy_names_no_buffer():
    destroy = body(CODE, CODE.index("void pbf_destroy(pbf_ctx *ctx)"))
    assert "delete ctx;" in destroy and "hipStreamSynchronize" in destroy and "hipSetDevice" in destroy
    assert not re.search(MEMBER_ADDRESS, destroy), re.findall(r"[^\n]*" + MEMBER_ADDRESS + r"[^\n]*", destroy)
    assert "hipFree" not in destroy and "hipHostFree" not in destroy


def test_device_memory_is_freed_by_its_owner_only():
    where = enclosing(CODE, DEVICE_FREE)
    assert where and "DevBuf" in where and set(where) <= {"DevBuf", "ensure"}, where


def test_pinned_memory_is_allocated_and_freed_by_its_owner_only():
    where = enclosing(CODE, PINNED_CALL)
    assert where.count("Pinned") >= 2, where
    assert all(name == "Pinned" or name.startswith("pbf_comm_") for name in where), where


def test_a_buffer_cannot_be_copied():
    assert re.search(DELETED_COPY, body(CODE, CODE.index("struct DevBuf")))


def test_the_regular_expressions_see_a_bad_example():
    for bad in ["DevBuf *all[] = {&ctx->pos4[0], &ctx->pos4[1]};", "free_it(& ctx -> wells);"]:
        assert re.search(MEMBER_ADDRESS, bad), bad
    for ok in ["if (ctx->regPtr) (void)hipHostUnregister(ctx->regPtr);", "if (a && ctx->b) return;"]:
        assert not re.search(MEMBER_ADDRESS, ok), ok
    assert re.search(DELETED_COPY, "  DevBuf(const DevBuf &) = delete;") and re.search(DELETED_COPY, "DevBuf( const DevBuf& o )=delete;")
    assert not re.search(DELETED_COPY, "  DevBuf(DevBuf &&o) noexcept;") and not re.search(DELETED_COPY, "DevBuf(const DevBuf &) = default;")
    sample = """
struct Owner {
  ~Owner() { if (p) (void)hipFree(p); }
};
template <typename T> struct Host {
  void reset() { (void)hipHostFree(p); }
};
int release(pbf_ctx *ctx, DevBuf &b) {
  if (b.p) HIPCHK(ctx, hipFree (b.p));
  return PBF_OK;
}
void pbf_comm_destroy(pbf_comm *c) {
  for (void *h : c->host) (void)hipHostFree(h);
}
static int stray = hipHostMalloc(&q, 64, 0);
"""
    assert enclosing(sample, DEVICE_FREE) == ["Owner", "release"]
    assert enclosing(sample, PINNED_CALL) == ["Host", "pbf_comm_destroy", ""]
    assert body("void f() { a { b } c }", 0) == " a { b } c "
