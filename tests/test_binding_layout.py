"""Where the HIP sources keep their cross-file signatures and their launches
(source text only, no GPU and no compiler): ``launch.h`` declares every
function that crosses a file boundary once, each is defined in exactly one
``.hip`` file that includes the header (so a mismatch is a compile error), and
``bindings.hip`` neither redeclares anything nor launches a kernel itself."""

import re
from pathlib import Path

HIP = Path(__file__).resolve().parents[1] / "kllms_amd" / "ops" / "hip"

# A cross-file function is named launch_*, ipc_ar_* or *_plan, whatever it
# returns and however it is indented. After comments are stripped, a mention
# whose parameter list runs into ";" is a declaration (or a call), one that
# runs into "{" a definition.
_NAME = r"\b((?:launch_|ipc_ar_)\w+|\w+_plan)\s*\("
_DECL = re.compile(_NAME + r"[^;{}]*;")
_DEFN = re.compile(_NAME + r"[^;{}]*\{")
_COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)


def _code(path):
    return _COMMENT.sub("", path.read_text())


def _sources():
    # *_hip.hip are build-time copies torch's extension builder leaves behind
    return {p.name: _code(p) for p in sorted(HIP.glob("*.hip"))
            if not p.name.endswith("_hip.hip")}


def _header_block():
    """The text between the braces of launch.h's one linkage block."""
    text = _code(HIP / "launch.h")
    head = 'extern "C" {'
    assert text.count(head) == 1
    return text[text.index(head) + len(head):text.rindex("}")]


def _declared():
    return _DECL.findall(_header_block())


def test_bindings_declare_and_launch_nothing():
    text = _sources()["bindings.hip"]
    for word in ("extern", "__global__", "hipLaunchKernelGGL", "<<<"):
        assert word not in text, f"bindings.hip contains {word!r}"
    assert '#include "launch.h"' in text


def test_launch_h_depends_on_common_h_only():
    includes = re.findall(r'^#include\s+(\S+)', (HIP / "launch.h").read_text(), re.M)
    assert includes == ['"common.h"']


def test_every_declared_function_is_defined_once_under_its_declaration():
    declared = _declared()
    assert len(declared) == len(set(declared)), "a function is declared twice in launch.h"
    # every statement of the block is a declaration the pattern knows: nothing
    # with another kind of name is declared behind these tests' back
    assert len(declared) == _header_block().count(";"), declared
    assert "launch_rmsnorm" in declared and "ipc_ar_create" in declared \
        and "linear_fp8w_plan" in declared, declared
    sources = _sources()
    for name in declared:
        homes = [f for f, text in sources.items() for n in _DEFN.findall(text) if n == name]
        assert len(homes) == 1, f"{name} is defined in {homes}"
        assert '#include "launch.h"' in sources[homes[0]], \
            f"{homes[0]} defines {name} without including launch.h"


def test_every_launcher_and_plan_is_declared():
    """Nothing crosses a file boundary behind the header's back: the launch_*,
    *_plan and ipc_ar_* definitions are exactly the declared ones."""
    declared = set(_declared())
    for f, text in _sources().items():
        for name in _DEFN.findall(text):
            assert name in declared, f"{f} defines {name}, which launch.h does not declare"
