"""The Python side of the resident feed's plumbing: ``feed.Feed`` (the order rows, boxes, mix, aug, keep, ra as one value) and
``engine.forward_call`` (which cara_vit_forward* entry a forward calls, with which arguments), the latter against two documents it
does not read: the prototypes of include/cara_hip.h and the argtypes of cara_amd/_lib.py.  CPU only."""
import ctypes as C
import itertools
import re

import pytest
import torch

from cara_amd import _lib
from cara_amd._lib import CaraError
from cara_amd.engine import forward_call
from cara_amd.feed import Feed
from tests.test_abi_docs import HDR, _strip_comments

TABLES = ("boxes", "mix", "aug", "keep", "ra")
PATTERNS = [p for n in range(len(TABLES) + 1) for p in itertools.combinations(TABLES, n)]


def test_item_round_trip_for_every_presence_pattern():
    assert len(PATTERNS) == 32 and Feed._fields == ("rows", *TABLES)
    rows = torch.arange(4)
    for present in PATTERNS:
        f = Feed(rows, **{n: torch.full((4, 1), i, dtype=torch.int32) for i, n in enumerate(TABLES) if n in present})
        item = f.item()
        if not present:
            assert item is rows
        else:
            assert isinstance(item, tuple) and len(item) == 1 + max(1 + TABLES.index(n) for n in present)
            assert all((t is None) == (n not in present) for n, t in zip(TABLES, item[1:]))
        back = Feed.of(item)
        assert all(a is b for a, b in zip(back, f)), present
        assert Feed.of(list(item) if present else [item]) == back
        assert tuple(f.tables()) == present and all(f.tables()[n] is getattr(f, n) for n in present)
        assert len(f.static()) == 1 + len(present) and f.static()[0] is rows and all(a is b for a, b in zip(f.static()[1:], f.tables().values()))
    with pytest.raises(CaraError, match="7 entries"):
        Feed.of((rows, None, None, None, None, None, None))
    with pytest.raises(CaraError):
        Feed.of(())


def header_prototype(name):
    """[(parameter, "int" or "pointer")] of ``int name(...);`` in include/cara_hip.h"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^()]*)\)\s*;", _strip_comments(HDR))
    assert m, name
    out = []
    for decl in m.group(1).split(","):
        decl = " ".join(decl.split())
        base, stars, param = re.fullmatch(r"((?:const\s+)?(?:unsigned\s+)?\w+)\s*(\**)\s*(\w+)", decl).groups()
        assert stars or base == "int", decl
        out.append((param, "pointer" if stars else "int"))
    return out


# the entry named after the last table present in the order boxes < mix < aug < keep < ra, written out
ENTRY = {
    (): "cara_vit_forward_u8_rows",
    ("boxes",): "cara_vit_forward_u8_rows_crop",
    ("mix",): "cara_vit_forward_u8_rows_mix", ("boxes", "mix"): "cara_vit_forward_u8_rows_mix",
    ("aug",): "cara_vit_forward_u8_rows_aug", ("boxes", "aug"): "cara_vit_forward_u8_rows_aug",
    ("mix", "aug"): "cara_vit_forward_u8_rows_aug", ("boxes", "mix", "aug"): "cara_vit_forward_u8_rows_aug",
    ("keep",): "cara_vit_forward_u8_rows_keep", ("boxes", "keep"): "cara_vit_forward_u8_rows_keep",
    ("mix", "keep"): "cara_vit_forward_u8_rows_keep", ("aug", "keep"): "cara_vit_forward_u8_rows_keep",
    ("boxes", "mix", "keep"): "cara_vit_forward_u8_rows_keep", ("boxes", "aug", "keep"): "cara_vit_forward_u8_rows_keep",
    ("mix", "aug", "keep"): "cara_vit_forward_u8_rows_keep", ("boxes", "mix", "aug", "keep"): "cara_vit_forward_u8_rows_keep",
}
ENTRY.update({(*p, "ra"): "cara_vit_forward_u8_rows_ra" for p in list(ENTRY)})   # ... and ra is the last of all

INTS = {"n_split": 1000, "Hs": 48, "Ws": 40}


def _values(source):
    """a distinct stand-in for every parameter that is not a table ("images" or "pixels" says which kind of batch it is)"""
    names = ("g", "s", "w", "cp", "head_w", "head_b", source, "rows", "mean", "std", "droppath", "workspace", "logits", "bad", "stream",
             "stat_scratch", "ra_scratch")
    return {**{n: f"<{n}>" for n in names}, **INTS}


def _check_against_the_documents(entry, params, tables):
    proto = header_prototype(entry)
    assert [n for n, _ in params] == [n for n, _ in proto], (entry, params)
    # (an entry without stated argtypes takes pointers only: ctypes' default for the c_void_p the engine hands over)
    argtypes = getattr(_lib.lib(), entry).argtypes or [C.c_void_p] * len(proto)
    assert len(params) == len(argtypes)
    for (n, v), (_, kind), at in zip(params, proto, argtypes):
        assert (kind == "int") == (at is C.c_int) == isinstance(v, int), (entry, n, kind, at, v)
        want = tables[n] if n in tables else None if n in TABLES or (n == "stat_scratch" and "aug" not in tables) else INTS.get(n, f"<{n}>")
        assert v is want or v == want, (entry, n, v, want)


def test_entry_and_arguments_for_every_presence_pattern():
    assert sorted(ENTRY) == sorted(PATTERNS)
    for present in PATTERNS:
        tables = {n: f"<table {n}>" for n in present}
        entry, params = forward_call(tables, _values("pixels"))
        assert entry == ENTRY[present], present
        _check_against_the_documents(entry, params, tables)
        got = dict(params)
        assert ("stat_scratch" in got and got["stat_scratch"] is not None) == ("aug" in present), present
        assert ("ra_scratch" in got and got["ra_scratch"] is not None) == ("ra" in present), present


def test_entry_and_arguments_for_an_fp32_batch():
    for tables, want in (({}, "cara_vit_forward"), ({"keep": "<table keep>"}, "cara_vit_forward_keep")):
        entry, params = forward_call(tables, _values("images"))
        assert entry == want
        _check_against_the_documents(entry, params, tables)
    with pytest.raises(CaraError, match="keep table only"):
        forward_call({"mix": "<table mix>"}, _values("images"))
