"""The suite's own shape: a module-level function or class defined twice in a
test module silently replaces the first definition, so a test of that name
stops running (pytest collects the module's final namespace). Every
tests/*.py is parsed and such a name fails here."""
import ast
import collections
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def duplicate_definitions(source, filename="<string>"):
    """Names bound more than once by a def / async def / class statement in the
    module's own body, with their lines."""
    seen = collections.defaultdict(list)
    for node in ast.parse(source, filename).body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            seen[node.name].append(node.lineno)
    return {name: lines for name, lines in seen.items() if len(lines) > 1}


def test_no_module_level_name_is_defined_twice():
    files = sorted(glob.glob(os.path.join(HERE, "*.py")))
    assert len(files) > 10, files
    bad = {}
    for path in files:
        with open(path, encoding="utf-8") as f:
            dup = duplicate_definitions(f.read(), path)
        if dup:
            bad[os.path.basename(path)] = dup
    assert not bad, bad


def test_the_check_sees_a_shadowed_test():
    src = "def test_a():\n    pass\n\n\nclass T:\n    pass\n\n\ndef test_a():\n    pass\n"
    assert duplicate_definitions(src) == {"test_a": [1, 9]}
    assert duplicate_definitions("def a():\n    def b():\n        pass\n    def b():\n        pass\n") == {}
