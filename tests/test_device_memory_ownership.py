"""CPU: who returns device memory in natac_api.hip.  Pool blocks go back only through the owner type (PoolBuf) and the pool itself;
hipFree is the pool's, plus the clock trace's sampler buffer (d_ck), which relies on hipFree's implicit device synchronisation."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nucleoatac_amd", "csrc", "natac_api.hip")


def code_only(src):
    """comments blanked (line numbers kept), string literals left as they are"""
    def blank(m):
        t = m.group(0)
        return t if t.startswith('"') else re.sub(r"[^\n]", " ", t)
    return re.sub(r'"(?:\\.|[^"\\\n])*"|//[^\n]*|/\*.*?\*/', blank, src, flags=re.S)


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


def test_pool_blocks_are_freed_only_by_their_owner():
    code = code_only(open(SRC).read())
    pool = pool_span(code)
    owner = braced(code, "class PoolBuf {")
    assert [arg for _, arg in calls(code[slice(*owner)], "dev_free")] == ["p_"]      # reset(): the one way a block goes back
    rest = outside(code, [pool, owner])
    assert calls(rest, "dev_free") == [], "dev_free outside PoolBuf and the pool (line, argument)"


def test_hip_free_only_in_pool_and_clock_trace():
    code = code_only(open(SRC).read())
    pool = pool_span(code)
    assert len(calls(code[slice(*pool)], "hipFree")) >= 2          # the pool's own: trim and the uncached free
    stray = [(line, arg) for line, arg in calls(outside(code, [pool]), "hipFree") if arg != "c->d_ck"]
    assert stray == [], "hipFree outside the pool and the clock trace (line, argument)"
