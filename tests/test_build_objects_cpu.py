"""icem_amd.build names an object by what it is compiled from, not by where the tree lies."""
import os
import shutil


def test_object_names_do_not_depend_on_the_path_of_the_tree(tmp_path, monkeypatch):
    """A built tree that is copied or moved must keep objects that object_path() finds (test_chain_isa_cpu.py and
    test_register_hygiene_cpu.py read them; with the include path in the key they errored there instead of passing)."""
    from icem_amd import build as B
    here = [os.path.basename(B.object_path(u)) for u in B.UNITS]
    root = tmp_path / "elsewhere"
    csrc = root / "icem_amd" / "csrc"
    csrc.mkdir(parents=True)
    for f in os.listdir(B.CSRC):
        if f.endswith((".hip", ".h")):
            shutil.copy(os.path.join(B.CSRC, f), csrc / f)
    (root / "include").mkdir()
    shutil.copy(os.path.join(os.path.dirname(B.HERE), "include", "icem_hip.h"), root / "include" / "icem_hip.h")
    monkeypatch.setattr(B, "HERE", str(root / "icem_amd"))
    monkeypatch.setattr(B, "CSRC", str(csrc))
    monkeypatch.setattr(B, "OBJ", str(csrc / "_obj"))
    there = [B.object_path(u) for u in B.UNITS]
    assert all(p.startswith(str(csrc)) for p in there)
    assert [os.path.basename(p) for p in there] == here
