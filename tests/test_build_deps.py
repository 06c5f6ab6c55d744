"""buildlib.needs_build() must watch every header the library is compiled from: a header it does not know can be edited and the stale
libokenv.so stays, and the suite then passes on code it did not compile."""
import os
import re

from openkitchen_amd import buildlib

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def reached_headers():
    """The project's own headers okenv_capi.hip includes, transitively: each #include "..." resolved as the compiler resolves it, against
    the including file's directory and then the -I directories of buildlib.build()."""
    search = [os.path.join(buildlib.ROOT, "include"), buildlib.CSRC]
    todo, seen, unresolved = list(buildlib.HIP_SOURCES), set(), []
    while todo:
        path = todo.pop()
        with open(path) as f:
            text = f.read()
        for name in INCLUDE.findall(text):
            hits = [os.path.normpath(os.path.join(d, name)) for d in [os.path.dirname(path)] + search]
            hits = [h for h in hits if os.path.exists(h)]
            if not hits:
                unresolved.append((path, name))
            elif hits[0] not in seen:
                seen.add(hits[0])
                todo.append(hits[0])
    return seen, unresolved


def test_needs_build_watches_every_header_the_library_includes():
    reached, unresolved = reached_headers()
    assert not unresolved, unresolved
    assert os.path.join(buildlib.CSRC, "ok_qcnn.h") in reached  # (the walk itself works)
    watched = {os.path.normpath(p) for p in buildlib.sources() + buildlib.headers()}
    assert sorted(reached - watched) == []


def test_a_newer_header_asks_for_a_build(monkeypatch):
    """With a library of time 1 and every source of time 0, only the touched header (time 2) can ask for the build."""
    touched = [None]
    monkeypatch.setattr(os.path, "exists", lambda p, exists=os.path.exists: p == buildlib.LIB_PATH or exists(p))
    monkeypatch.setattr(os.path, "getmtime", lambda p: 1.0 if p == buildlib.LIB_PATH else (2.0 if p == touched[0] else 0.0))
    assert not buildlib.needs_build()
    touched[0] = os.path.join(buildlib.CSRC, "ok_qcnn.h")
    assert buildlib.needs_build()
