"""The layers of the package's stages, read off the source: tables and clr_model below, gallery and
resegmentation on them, linking on gallery, pipeline on all.  No module among them imports a module of
the package inside a function body (where a cycle can hide), the package's top-level import graph has no
cycle, and each stage module imports on its own in a fresh interpreter."""
import ast
import os
import subprocess
import sys

import pytest

from helpers import ROOT

PKG = 'speaker-diarization_amd'
STAGES = ('tables', 'clr_model', 'gallery', 'resegmentation', 'linking', 'pipeline')


def _modules():
    return sorted(f[:-3] for f in os.listdir(os.path.join(ROOT, PKG)) if f.endswith('.py') and f != '__init__.py')


def _package_imports(name):
    """(at the top level, inside function bodies): the package's modules that module `name` imports by a
    relative import -- `from . import a`, `from .a import b` -- each a set of module names."""
    known = set(_modules())
    tree = ast.parse(open(os.path.join(ROOT, PKG, name + '.py')).read())
    top, inner = set(), set()

    def walk(node, into):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.ImportFrom) and child.level == 1:
                into.update([child.module.split('.')[0]] if child.module else [a.name for a in child.names])
            assert not (isinstance(child, ast.ImportFrom) and child.level > 1), '%s: an import from above the package' % name
            walk(child, inner if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)) else into)

    walk(tree, top)
    return top & known, inner & known


def test_the_stage_modules_exist_and_pipeline_keeps_their_names():
    assert set(STAGES) <= set(_modules())
    from conftest import pkg
    pipeline = pkg('pipeline')
    for mod, names in (('tables', ('BatchFile', '_turn_table', '_segment_ranges', 'link_speakers')),
                       ('linking', ('LINK_CL', 'LINK_CLR', 'link_batch', 'ubm_ranges', '_link_model')),
                       ('clr_model', ('LINK_CLR', 'ubm_ranges', '_link_model'))):
        for n in names:
            assert getattr(pipeline, n) is getattr(pkg(mod), n), (mod, n)


@pytest.mark.parametrize('name', STAGES)
def test_no_package_import_inside_a_function_body(name):
    assert _package_imports(name)[1] == set()


def test_the_top_level_import_graph_has_no_cycle():
    graph = {m: _package_imports(m)[0] for m in _modules()}
    assert graph['tables'] == {'hipabi'} and graph['clr_model'] == {'hipabi'}
    assert 'pipeline' not in graph['gallery'] | graph['resegmentation'] | graph['linking']
    done, path = set(), []

    def visit(m):
        assert m not in path, 'import cycle: %s' % ' -> '.join(path[path.index(m):] + [m])
        if m in done:
            return
        path.append(m)
        for dep in sorted(graph[m]):
            visit(dep)
        path.pop()
        done.add(m)

    for m in graph:
        visit(m)


@pytest.mark.parametrize('name', ['gallery', 'resegmentation', 'linking'])
def test_a_stage_module_imports_alone_in_a_fresh_interpreter(name):
    code = ('import importlib, sys; sys.path.insert(0, %r); importlib.import_module(%r); '
            'assert %r not in sys.modules' % (ROOT, PKG + '.' + name, PKG + '.pipeline'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
