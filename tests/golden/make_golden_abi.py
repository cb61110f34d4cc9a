#!/usr/bin/env python3
"""Mint abi_tables.json: what coevonet_amd/lib.py binds, rendered as data - for every ``_SIGS`` entry the restype and
argtypes by ctypes type name (``POINTER(X)`` rendered as such, a struct by value by its class name), for every
``ctypes.Structure`` mirror its ``sizeof`` and each field's name, type name, offset and size, and the module constants that
mirror ``COEVO_*`` values (``ST_NAMES`` by its keys, the two task dtypes by their ``descr``).  Needs neither libcoevo.so nor
a GPU.

    python tests/golden/make_golden_abi.py       # writes the fixture, or checks the tree against it when it exists

The fixture was minted at the commit BEFORE lib.py derived these tables from include/coevo.h, when ``_SIGS``, the fourteen
``_fields_`` lists and the integers were written out by hand.  DO NOT REGENERATE it from a tree that derives them:
tests/test_abi.py compares the derived tables with it, and names the five argument positions that were ``POINTER(...)``
then and are ``c_void_p`` now.
"""
import ctypes as ct
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FIXTURE = os.path.join(HERE, "abi_tables.json")
STRUCTS = ("PCG64State", "PerturbJob", "Perturb16Job", "FinalizeJob", "ResetSeg", "FinalPack", "RolloutDesc", "HostCohort",
           "HostRolloutDesc", "FrameCohort", "FramesRolloutDesc", "GaSelectRole", "GaAdaptArgs", "GaPromoteRole")
CONSTANTS = ("OBS_STRIDE", "LOGIT_STRIDE", "FC_MAX_ROWS", "MPE_STATE_DOUBLES", "STAMP_SLOTS", "DQN_LOGIT_STRIDE",
             "DQN_FC1_TILED", "DQP_SKIP_BN", "DQN_MAX_ROWS", "TASK_RESIDENT", "TASK_TILED", "TASK_TWIN_SHIFT",
             "TASK_TWIN_UNIT", "W2_FLOATS")


def type_name(t):
    """c_int and c_int32 are one class in ctypes, so a name is the class's own: two renderings agree iff the types do"""
    if t is None:
        return "None"
    if isinstance(t, type) and issubclass(t, ct._Pointer):
        return f"POINTER({type_name(t._type_)})"
    if isinstance(t, type) and issubclass(t, ct.Array):
        return f"{type_name(t._type_)}[{t._length_}]"
    return t.__name__


def render(L):
    sigs = {name: {"restype": type_name(res), "argtypes": [type_name(a) for a in args]}
            for name, (res, args) in sorted(L._SIGS.items())}
    structs = {}
    for name in STRUCTS:
        cls = getattr(L, name)
        structs[name] = {"sizeof": ct.sizeof(cls),
                         "fields": [[f, type_name(t), getattr(cls, f).offset, getattr(cls, f).size] for f, t in cls._fields_]}
    consts = {name: int(getattr(L, name)) for name in CONSTANTS}
    consts["ST_NAMES"] = sorted(L.ST_NAMES)
    for name in ("TASK_DTYPE", "DQN_TASK_DTYPE"):
        dt = getattr(L, name)
        consts[name] = {"itemsize": dt.itemsize, "fields": [[f, dt.fields[f][0].str, dt.fields[f][1]] for f in dt.names]}
    return {"sigs": sigs, "structs": structs, "constants": consts}


def main():
    from coevonet_amd import lib as L
    got = render(L)
    if not os.path.exists(FIXTURE):
        with open(FIXTURE, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {FIXTURE}: {len(got['sigs'])} entry points, {len(got['structs'])} structs")
        return 0
    want = json.load(open(FIXTURE))
    diffs = [f"{name}[{i}]: {a} -> {b}" for name in want["sigs"]
             for i, (a, b) in enumerate(zip(want["sigs"][name]["argtypes"], got["sigs"].get(name, {}).get("argtypes", [])))
             if a != b]
    same = json.loads(json.dumps(got)) == want
    print("identical to the fixture" if same else "differs from the fixture:\n  " + "\n  ".join(diffs or ["(not in an argtype)"]))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
