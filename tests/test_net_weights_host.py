"""The declaration of the network's arrays (n-hans_amd/csrc/net_weights.h) on the host, against what fold.fold_arrays emits:
tests/net_weights_main.cpp includes the header alone, resolves the "name count" lists it is fed over fake distinct pointers
and prints every field of the struct with the name of the array it points at, or the refusal.  Built with the address and
undefined-behaviour sanitizers and run as a plain child process; one run takes all the blobs of a test.  Only names and
sizes are needed, so no weights reach the program."""
import os
import re
import subprocess

import pytest

import nhans_amd  # noqa: F401
from nhans_amd import fold

HERE = os.path.dirname(os.path.abspath(__file__))

# Arrays the folder writes and the library deliberately never reads, each with its reason: none.
UNREAD = {}

SUFFIX = {"wpk[0]": ".wpk", "wpk[1]": ".wpk_h", "wpk_t[0]": ".wpk_t", "wpk_t[1]": ".wpk_t_h", "w": ".w", "cb": ".cb", "tf": ".tf",
          "tt": ".tt", "ff": ".ff", "idw": ".idw", "ws": ".ws", "wino_u": ".wino", "wino_ws": ".wino.ws"}
SINGLE = {"zero": "zero", "tw400": "tw400", "window": "window", "wsyn": "wsyn", "cond_w": "cond.w", "cond_base": "cond.base",
          "ones": "head.dense.idw"}


def expected_name(field):
    """The array a field of NetWeights must point at, from the field's own label (the test's restatement of the naming)."""
    if field in SINGLE:
        return SINGLE[field]
    m = re.fullmatch(r"(tower|stack)\[(\d)\]\.(c[12])\.(.+)", field)
    if m:
        return "%s%s.%s%s" % ("t" if m.group(1) == "tower" else "m", m.group(2), m.group(3), SUFFIX[m.group(4)])
    m = re.fullmatch(r"head_(conv|dense)\.(.+)", field)
    return "head.%s%s" % (m.group(1), SUFFIX[m.group(2)])


def is_optional(name):
    return name.endswith((".tt", ".ff", ".wino", ".wino.ws"))


def is_split(name):
    return not is_optional(name) and name.endswith(("_h", ".ws"))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("net_weights") / "net_weights_main")
    # (the sanitizer runtimes are linked statically, so the program needs no preload)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", os.path.join(HERE, "net_weights_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr

    def resolve(blobs):
        """blobs: list of {name: count} -> per blob ("refused", message) or ("ok", has_split, {field: name})"""
        text = "".join("".join("%s %d\n" % kv for kv in b.items()) + "--\n" for b in blobs)
        run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        chunks = run.stdout.split("--\n")
        assert len(chunks) == len(blobs) + 1 and chunks[-1] == ""
        out = []
        for ch in chunks[:-1]:
            lines = ch.splitlines()
            if lines[0].startswith("refused: "):
                assert len(lines) == 1
                out.append(("refused", lines[0][len("refused: "):]))
                continue
            fields = dict(ln.split(" = ") for ln in lines[1:])
            assert len(fields) == len(lines) - 1
            out.append(("ok", {"has_split = 0": False, "has_split = 1": True}[lines[0]], fields))
        return out

    return resolve


@pytest.fixture(scope="module")
def sizes(weights_denoiser, weights_separator):
    """{(kind, split_f16): {name: float count}} of what the folder emits for the synthetic weights"""
    return {(kind, split): {k: v.size for k, v in fold.fold_arrays(W, kind, split).items()}
            for kind, W in (("denoiser", weights_denoiser), ("separator", weights_separator)) for split in (True, False)}


def refusal(name, count):
    return "folded blob: array '%s' missing or wrong size (want %d)" % (name, count)


def without(blob, *names):
    return {k: v for k, v in blob.items() if k not in names}


def test_the_full_set_resolves_and_every_emitted_array_is_declared(program, sizes):
    """(a) every pointer of the struct is the array of the right name; (f) every array the folder writes lands in a field."""
    keys = list(sizes)
    for key, res in zip(keys, program([sizes[k] for k in keys])):
        assert res[0] == "ok", (key, res)
        _, has_split, fields = res
        assert has_split == key[1]
        for field, name in fields.items():
            assert name == expected_name(field), (key, field, name)
        unread = set(sizes[key]) - set(fields.values())
        assert unread == set(UNREAD), (key, sorted(unread))
        # (one field per array, except that nothing forbids two: none today)
        assert len(set(fields.values())) == len(fields)


def test_each_required_array_removed_in_turn_is_refused_by_name(program, sizes):
    """(b), for the f32-only blob and the split one."""
    for key, blob in sizes.items():
        req = [n for n in blob if not is_optional(n) and not is_split(n)]
        assert len(req) > 60
        for name, res in zip(req, program([without(blob, n) for n in req])):
            assert res == ("refused", refusal(name, blob[name])), (key, name, res)


def test_split_arrays_are_required_exactly_when_the_blob_carries_split_weights(program, sizes):
    """(c) `head.dense.wpk_h` is the mark: with it every `*_h` and `<conv>.ws` is required, without it none is asked for."""
    for kind in ("denoiser", "separator"):
        blob = sizes[(kind, True)]
        split = [n for n in blob if is_split(n)]
        assert len(split) > 50 and "m3.c1.wpk_h" in split and "t2.c2.ws" in split and "head.dense.ws" in split
        others = [n for n in split if n != "head.dense.wpk_h"]
        for name, res in zip(others, program([without(blob, n) for n in others])):
            assert res == ("refused", refusal(name, blob[name])), (kind, name, res)
        # without the mark: the other split arrays present (and unread), or absent
        for res in program([without(blob, "head.dense.wpk_h"), without(blob, *split)]):
            assert res[0] == "ok" and res[1] is False, res
            assert not [f for f in res[2] if f.endswith("[1]") or f.endswith(".ws")], res[2]
            assert not [n for n in res[2].values() if is_split(n)]


def test_every_array_one_float_short_is_refused_by_name(program, sizes):
    """(d) required and split arrays as if missing; optional ones for being present at a wrong size."""
    for key, blob in sizes.items():
        names = list(blob)
        for name, res in zip(names, program([dict(blob, **{n: blob[n] - 1}) for n in names])):
            assert res[0] == "refused" and "'%s'" % name in res[1] and "(want %d)" % blob[name] in res[1], (key, name, res)
            if not is_optional(name):
                assert res[1] == refusal(name, blob[name])


def test_optional_pairs_resolve_as_both_or_neither(program, sizes):
    """(e) `.tt` + `.ff` and `.wino` + `.wino.ws`: all removed, or one of a pair removed, leaves both fields of that conv null
    and every other field as it was."""
    blob = sizes[("denoiser", True)]
    (_, _, full), = program([blob])
    cases = [
        ([n for n in blob if n.endswith((".tt", ".ff"))], [f for f in full if f.endswith((".tt", ".ff"))]),
        ([n for n in blob if n.endswith((".wino", ".wino.ws"))], [f for f in full if f.endswith((".wino_u", ".wino_ws"))]),
        (["m3.c1.tt"], ["stack[3].c1.tt", "stack[3].c1.ff"]),
        (["m0.c1.ff"], ["stack[0].c1.tt", "stack[0].c1.ff"]),
        (["m1.c2.wino"], ["stack[1].c2.wino_u", "stack[1].c2.wino_ws"]),
        (["m2.c2.wino.ws"], ["stack[2].c2.wino_u", "stack[2].c2.wino_ws"]),
    ]
    assert len(cases[0][1]) == 32 and len(cases[1][1]) == 12
    for (removed, gone), res in zip(cases, program([without(blob, *r) for r, _ in cases])):
        assert res[0] == "ok" and res[1] is True, (removed, res)
        assert set(gone) <= set(full)
        assert res[2] == {f: n for f, n in full.items() if f not in gone}, removed
