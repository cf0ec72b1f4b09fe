"""The refusal of every create entry point for every family, pinned message by message (no GPU: a configuration refusal comes
before the device lookup).

A cell is (call form, family id): the entry is called with a zeroed ``s3enc_config`` whose only set field is ``family``, a
zeroed block of the entry's own type, a zero-length tensor array and device 0.  Every cell is a refusal: a non-zero return, a
null handle and the message recorded in ``tests/golden/create_refusals.json``.  The ``null:`` forms pass a null block to the
entries that require one and expect their "null argument" refusal whatever the family.

``python tests/test_family_dispatch_cpu.py`` re-records the file from the library that is built (done once, from the commit
before the family table went in).
"""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "create_refusals.json")

N_FAMILIES = 14
# the entries that take a second configuration block, in the order they were added, with the ctypes struct of the block
BLOCK_ENTRIES = [("s3enc_create_ex", "S3Wav2vecConfig"), ("s3enc_create_cpc", "S3CpcConfig"), ("s3enc_create_apc", "S3ApcConfig"),
                 ("s3enc_create_mockingjay", "S3MockingjayConfig"), ("s3enc_create_decoar", "S3DecoarConfig"),
                 ("s3enc_create_npc", "S3NpcConfig"), ("s3enc_create_vggish", "S3VggishConfig"),
                 ("s3enc_create_byol_a", "S3ByolAConfig"), ("s3enc_create_mae_ast", "S3MaeAstConfig")]
# call form -> (entry, block struct or None, pass the block as null)
FORMS = {"s3enc_create": ("s3enc_create", None, False), "s3enc_create_ex(null)": ("s3enc_create_ex", "S3Wav2vecConfig", True)}
FORMS.update({entry: (entry, block, False) for entry, block in BLOCK_ENTRIES})
FORMS.update({"null:" + entry: (entry, block, True) for entry, block in BLOCK_ENTRIES[1:]})  # (s3enc_create_ex takes null as legal)
CELLS = [(form, family) for form in FORMS for family in range(N_FAMILIES)]


def call(form, family):
    """-> (return code, handle value or None, s3enc_last_error())"""
    from s3prl_amd import _lib

    lib = _lib.load()
    entry, block, null = FORMS[form]
    ccfg = _lib.S3Config()
    ccfg.family = family
    tensors = (_lib.S3Tensor * 1)()
    h = C.c_void_p(0xDEAD)  # a refusal leaves a null handle behind, not the caller's old value
    args = [C.byref(ccfg)]
    if block is not None:
        args.append(None if null else C.byref(getattr(_lib, block)()))
    rc = getattr(lib, entry)(*args, tensors, 0, 0, C.byref(h))
    return rc, h.value, lib.s3enc_last_error().decode()


def test_the_matrix_is_whole():
    assert len([f for f in FORMS if not f.startswith("null:")]) == 11 and len(CELLS) == (11 + 8) * N_FAMILIES
    with open(GOLDEN) as f:
        assert set(json.load(f)) == {f"{form}|{family}" for form, family in CELLS}


@pytest.mark.parametrize("form,family", CELLS, ids=[f"{form}-{family}" for form, family in CELLS])
def test_create_refusal(form, family):
    with open(GOLDEN) as f:
        expected = json.load(f)[f"{form}|{family}"]
    rc, handle, msg = call(form, family)
    assert rc != 0 and msg == expected
    if form.startswith("null:"):  # (refused before the entry touches *out)
        assert msg == f"{FORMS[form][0]}: null argument"
    else:
        assert handle is None


if __name__ == "__main__":
    rec = {}
    for form, family in CELLS:
        rc, handle, msg = call(form, family)
        assert rc != 0, (form, family, "not a refusal")
        rec[f"{form}|{family}"] = msg
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cells")
