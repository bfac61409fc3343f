"""CPU: who takes and returns device memory in the library's translation unit (natac_api.hip and every csrc/*.hpp it includes).  Pool
blocks go back only through the owner type (PoolBuf, natac_runtime.hpp) and the pool itself; hipMalloc and hipFree are the pool's, plus
two owners outside it: DevBuf (natac_bgzf_dev.hpp), the device decoders' window owner -- a cached 8 GiB window would starve the
pipeline of the pool's memory -- and the clock trace's sampler buffer (d_ck), which relies on hipFree's implicit device synchronisation."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nucleoatac_amd", "csrc")
SOURCES = [os.path.join(CSRC, "natac_api.hip")] + sorted(glob.glob(os.path.join(CSRC, "*.hpp")))


def code_only(src):
    """comments blanked (line numbers kept), string literals left as they are"""
    def blank(m):
        t = m.group(0)
        return t if t.startswith('"') else re.sub(r"[^\n]", " ", t)
    return re.sub(r'"(?:\\.|[^"\\\n])*"|//[^\n]*|/\*.*?\*/', blank, src, flags=re.S)


def translation_unit():
    """{file name: its code}"""
    return {os.path.basename(p): code_only(open(p).read()) for p in SOURCES}


def braced(code, head):
    """[start, end) of the definition that begins with `head`, up to its matching closing brace"""
    start = code.index(head)
    depth, i = 0, code.index("{", start)
    while True:
        if code[i] == "{":
            depth += 1
        elif code[i] == "}":
            depth -= 1
            if depth == 0:
                return start, i + 1
        i += 1


def outside(code, spans):
    """code with the given spans blanked"""
    for a, b in spans:
        code = code[:a] + re.sub(r"[^\n]", " ", code[a:b]) + code[b:]
    return code


def pool_span(code):
    """the pool: from struct DevPool to the end of dev_free's definition"""
    return code.index("struct DevPool {"), braced(code, "static void dev_free(void *p) {")[1]


def calls(code, name):
    """(line, argument) of every call of `name` (its declarations, `void name(...)`, are not calls)"""
    return [(code.count("\n", 0, m.start()) + 1, m.group(1).strip())
            for m in re.finditer(r"(?<!void )\b%s\(([^()]*)\)" % name, code)]


def uses(code, name):
    """(line, the line's text) of every `name(`, whatever its arguments"""
    lines = code.split("\n")
    return [(n, lines[n - 1].strip()) for n in (code.count("\n", 0, m.start()) + 1 for m in re.finditer(r"\b%s\(" % name, code))]


def owners(tu):
    """{file name: spans of the code that may call the driver's allocator}: the pool and DevBuf"""
    return {"natac_runtime.hpp": [pool_span(tu["natac_runtime.hpp"])],
            "natac_bgzf_dev.hpp": [braced(tu["natac_bgzf_dev.hpp"], "struct DevBuf {")]}


def test_pool_blocks_are_freed_only_by_their_owner():
    tu = translation_unit()
    code = tu["natac_runtime.hpp"]
    pool = pool_span(code)
    owner = braced(code, "class PoolBuf {")
    assert [arg for _, arg in calls(code[slice(*owner)], "dev_free")] == ["p_"]      # reset(): the one way a block goes back
    tu["natac_runtime.hpp"] = outside(code, [pool, owner])
    stray = [(name, line, arg) for name, rest in tu.items() for line, arg in calls(rest, "dev_free")]
    assert stray == [], "dev_free outside PoolBuf and the pool (file, line, argument)"


def test_hip_free_only_in_pool_and_clock_trace():
    tu = translation_unit()
    own = owners(tu)
    pool = tu["natac_runtime.hpp"][slice(*own["natac_runtime.hpp"][0])]
    assert len(calls(pool, "hipFree")) >= 2          # the pool's own: trim and the uncached free
    assert len(uses(pool, "hipMalloc")) >= 2         # ... and the allocation with its retry after a trim
    devbuf = tu["natac_bgzf_dev.hpp"][slice(*own["natac_bgzf_dev.hpp"][0])]
    assert uses(devbuf, "hipMalloc") and uses(devbuf, "hipFree")      # DevBuf is an owner: it takes and returns its memory itself
    stray = []
    for name, code in tu.items():
        rest = outside(code, own.get(name, []))
        stray += [(name, line, arg) for line, arg in calls(rest, "hipFree") if arg != "c->d_ck"]
        # every hipFree is seen by calls(): none has nested parentheses in its argument
        assert len(calls(rest, "hipFree")) == len(uses(rest, "hipFree")), name
        stray += [(name, line, text) for line, text in uses(rest, "hipMalloc") if "&c->d_ck" not in text]
    assert stray == [], "hipFree / hipMalloc outside the pool, DevBuf and the clock trace (file, line, argument or text)"
