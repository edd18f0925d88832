"""CPU: the layout of the suite itself.  Test modules (``test_*.py``) import boxer_amd, oracle, third-party packages and
helper modules, never each other; what two of them share lives in a helper, a plain module in tests/ whose file name
pytest does not collect.  A helper imports no test module, defines nothing pytest would collect from a module that
imported it, and imports on a machine with no GPU and no built library."""
import ast
import glob
import os
import subprocess
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
MODULES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TESTS, "*.py")))
MODULES.remove("conftest")
HELPERS = [m for m in MODULES if not m.startswith("test_")]


def imported_modules(tree):
    """Every module an import statement names, at any depth of the file."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom):
            yield node.module or ""
            if not node.module:                      # from . import test_x
                for a in node.names:
                    yield a.name


def top_level_names(tree):
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            yield node.name
        elif isinstance(node, (ast.Import, ast.ImportFrom)):
            for a in node.names:
                yield a.asname or a.name.split(".")[0]
        elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            for target in (node.targets if isinstance(node, ast.Assign) else [node.target]):
                for n in ast.walk(target):
                    if isinstance(n, ast.Name):
                        yield n.id


def test_no_module_imports_a_test_module_and_no_helper_looks_like_a_test():
    assert HELPERS and len(HELPERS) < len(MODULES)
    for module in MODULES:
        tree = ast.parse(open(os.path.join(TESTS, module + ".py"), encoding="utf-8").read())
        for name in imported_modules(tree):
            assert not any(part.startswith("test_") for part in name.split(".")), \
                "%s.py imports the test module %s" % (module, name)
        if module in HELPERS:
            assert not module.endswith("_test"), "pytest would collect the helper %s.py as a test module" % module
            for name in top_level_names(tree):
                assert not name.startswith(("test", "Test")), \
                    "helper %s.py defines %s, which a test module importing it would collect" % (module, name)


CHILD = ("import sys; sys.path[:0] = [%r, %r]; import {0}; "
         "from boxer_amd import _lib; sys.exit(0 if _lib._lib is None else 3)" % (TESTS, ROOT))


@pytest.mark.parametrize("helper", HELPERS)
def test_helper_imports_alone_without_a_gpu_and_without_loading_the_library(helper):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    done = subprocess.run([sys.executable, "-c", CHILD.format(helper)], env=env, cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, "importing %s alone: exit %d (3: it loaded the library)\n%s" % (
        helper, done.returncode, done.stderr[-2000:])
