"""Every laboratory variant of tools/lab_variants.py still finds its anchors (text only, no compiler, no GPU).

A variant is a list of (file, old text, new text) patches of a copy of the product sources.  The product moves on; a variant
whose anchor text is gone used to go unnoticed until someone tried to build it on a GPU visit.  Here every entry of VARIANTS,
combinations expanded, is applied as text: every anchor must be found in the file its patch names, after the patches in front
of it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import lab_variants  # noqa: E402


def test_every_variant_is_listed_once_and_combos_name_variants():
    assert set(lab_variants.COMBOS) <= set(lab_variants.VARIANTS)
    for name, parts in lab_variants.COMBOS.items():
        assert parts and all(p in lab_variants.VARIANTS and p not in lab_variants.COMBOS for p in parts), name
    for name, (desc, patches) in lab_variants.VARIANTS.items():
        assert desc, name
        assert patches or name in lab_variants.COMBOS or name in lab_variants.DEFINE_VARIANTS, name   # (no variant without an effect)


@pytest.mark.parametrize("name", sorted(lab_variants.VARIANTS))
def test_every_anchor_is_found_in_its_file(name):
    from tssplat_amd import _build
    srcs = lab_variants.patched_sources(name)          # raises LookupError at the first anchor that is not found
    patches = [q for n in lab_variants.COMBOS.get(name, [name]) for q in lab_variants.VARIANTS[n][1]]
    assert set(srcs) == {f for f, _, _ in patches}
    for f, text in srcs.items():
        assert f in _build.SOURCES + _build.HEADERS, (name, f)
        original = open(os.path.join(_build.CSRC, f)).read()
        if name not in lab_variants.FLAG_VARIANTS:      # (a flag variant "patches" its file with itself to have it recompiled)
            assert text != original, (name, f)
