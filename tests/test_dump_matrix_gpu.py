"""tools/dump_matrix.py is how a refactor of the host code is compared with its parent bit for bit: two dumps of ONE tree must
compare identical, and its comparison must be able to fail."""
import importlib.util
import os

import numpy as np
import pytest

from util import ROOT

pytestmark = pytest.mark.gpu


def test_dump_matrix_is_reproducible_and_its_compare_can_fail(cuda, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("dump_matrix", os.path.join(ROOT, "tools", "dump_matrix.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for out in (a, b):
        tool.dump(out, ["captions_one", "llm_layer"])
    assert sorted(os.listdir(a)) == ["captions_one", "llm_layer"]
    capsys.readouterr()
    assert tool.compare(a, b) == 0
    assert capsys.readouterr().out.startswith("identical, 2 cases, ")
    # one element of one array flipped: named
    victim = os.path.join("captions_one", "shared.trim1.score.npy")
    x = np.load(os.path.join(b, victim))
    x.reshape(-1).view(np.uint32)[3] ^= 1
    np.save(os.path.join(b, victim), x)
    assert tool.compare(a, b) == 1
    assert capsys.readouterr().out.strip() == f"{victim}: 1 bytes differ"
    # a missing array is named too
    np.save(os.path.join(b, victim), np.load(os.path.join(a, victim)))
    os.remove(os.path.join(b, "llm_layer", "out.npy"))
    assert tool.compare(a, b) == 1
    assert capsys.readouterr().out.strip() == f"{os.path.join('llm_layer', 'out.npy')}: only in {a}"
