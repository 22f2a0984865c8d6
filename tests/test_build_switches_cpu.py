"""layout_constants.h says which build switches exist and that no other file defines one: held to that by reading the files."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRS = [os.path.join(ROOT, "ctucopy_amd", "csrc"), os.path.join(ROOT, "ctucopy_amd", "host")]
HOME = "layout_constants.h"
SWITCHES = ["CTU_STAMP"]  # every #ifndef CTU_... of layout_constants.h
# function-like macros of the kernels: statements of inline assembly and their operand selectors, not switches
# (and stream_plan.h's CTU_HOST_DEVICE, the `__host__ __device__` qualifier under hipcc and nothing under g++: no -D can set it)
MACROS = re.compile(r"CTU_(ADDTID16\w*|READ2_\w+|E_\w+|PC_ROW_BYTES|HOST_DEVICE)$")
DIRECTIVE = re.compile(r"^\s*#\s*(ifndef|define)\s+(CTU_\w*)", re.M)


def sources():
    for d in DIRS:
        for f in sorted(os.listdir(d)):
            if f.endswith((".h", ".cc", ".hip")):
                yield f, open(os.path.join(d, f)).read()


def include_guard(name, text):
    """`#ifndef X` directly followed by `#define X` as the file's first directives"""
    first = DIRECTIVE.findall(text)[:2]
    return len(first) == 2 and first[0] == ("ifndef", name) and first[1] == ("define", name)


def test_no_file_but_layout_constants_defines_a_switch():
    seen = 0
    stray = []
    for f, text in sources():
        seen += 1
        if f == HOME:
            continue
        for kind, name in DIRECTIVE.findall(text):
            if MACROS.match(name) or include_guard(name, text):
                continue
            stray.append("%s: #%s %s" % (f, kind, name))
    assert seen > 30, seen
    assert not stray, stray


def test_the_switches_of_layout_constants_are_the_listed_ones():
    text = open(os.path.join(DIRS[0], HOME)).read()
    found = [name for kind, name in DIRECTIVE.findall(text) if kind == "ifndef"]
    assert found == SWITCHES
    assert sorted(name for kind, name in DIRECTIVE.findall(text) if kind == "define") == sorted(SWITCHES)
