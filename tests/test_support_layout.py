"""Where test support lives: helpers shared by test modules are in plain modules of
tests/, so no module -- test, helper or tool -- imports from a test_*.py module."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPORT = re.compile(r"^\s*(?:from\s+test_\w+\s+import\b|import\s+(?:[\w.]+\s*,\s*)*test_\w+)", re.M)


def test_no_module_imports_from_a_test_module():
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "**", "*.py"),
                                                                      recursive=True)
    assert len(files) > 80, "the search found %d files: wrong root?" % len(files)
    found = []
    for path in sorted(files):
        with open(path) as f:
            text = f.read()
        for m in IMPORT.finditer(text):
            found.append("%s:%d: %s" % (os.path.relpath(path, ROOT), text.count("\n", 0, m.start()) + 1,
                                        m.group(0).strip()))
    assert not found, "imports from test modules (move the helper to a plain module of tests/):\n" + "\n".join(found)
