"""CPU: the build's input list (marl_sortingenv_amd/build.py: SOURCES + HEADERS, what staleness looks at) against the
`#include "..."` directives of the files it names.  Nothing is compiled."""
import glob
import os
import re

from marl_sortingenv_amd.build import HEADERS, PKG_DIR, REPO_ROOT, SOURCES

CSRC = os.path.join(PKG_DIR, "csrc")
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def test_every_quoted_include_names_a_build_input():
    inputs = {os.path.normpath(p) for p in SOURCES + HEADERS}
    checked = 0
    for path in sorted(inputs):
        if os.path.dirname(path) != CSRC:
            continue
        for name in INCLUDE.findall(open(path).read()):
            found = [p for p in (os.path.join(CSRC, name), os.path.join(REPO_ROOT, "include", name)) if os.path.isfile(p)]
            assert found, f'{os.path.basename(path)} includes "{name}", which is neither in csrc/ nor in include/'
            assert os.path.normpath(found[0]) in inputs, f'{os.path.basename(path)} includes "{name}", which build.py does not list'
            checked += 1
    assert checked, "no #include directive was found at all"


def test_every_header_in_csrc_is_a_build_input():
    listed = {os.path.normpath(p) for p in HEADERS}
    on_disk = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc"))
    assert on_disk
    missing = sorted(os.path.basename(p) for p in on_disk if os.path.normpath(p) not in listed)
    assert not missing, f"csrc/ files that build.py's HEADERS leave out: {missing}"
    assert all(os.path.isfile(p) for p in SOURCES + HEADERS)
