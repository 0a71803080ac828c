"""Writes tests/golden/text_frontend.json: the ids the REFERENCE's own text front end (models/parser.py of
vliu15/speech-masters-thesis) gives for the sentences below, without a dictionary (64 symbols) and with
tests/golden/tiny_cmudict.txt (148 symbols).  tests/test_text_frontend_cpu.py holds this repository's parser to them.

    python tests/golden/make_golden_text.py <path of a checkout of the reference>

The reference imports `inflect` and `unidecode`.  Neither is needed for what is captured here, so in-memory stand-ins are
installed first (as make_golden.py does for librosa): `unidecode` is the identity and refuses non-ASCII text, the inflect
engine raises when asked for a number.  The sentences are therefore ASCII and digit-free; number expansion and ASCII folding
are pinned by the tables of the test file instead."""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))

SENTENCES = [
    "Hello world.",
    "Dr. Smith met Mr. Jones at the co. office.",
    "Mrs. Brown and the Rev. Green went to St. Louis.",
    "btw the www page is down.",
    "{HH AH0 L OW1} world.",
    "Turn left on {HH AW1 S T AH0 N} Street.",
    "Say it again {W ER1 L D}",
    "Wait... what?! No way!!",
    "Two  spaces   here.",
    "A well-known state-of-the-art method.",
    "It's the doctor's way, isn't it?",
    "'Tis by the way.",
    "Printing, in the only sense with which we are at present concerned.",
    "(Parentheses) and: colons; semicolons.",
    "UPPER case And MiXeD.",
    "hello",
    "The http link and the src file use c++ and a dll.",
    "under_score and tilde~ and at@ sign.",
    "Lt. Col. Sanders, Esq. of Ft. Worth.",
    "  leading and trailing spaces  ",
    "{HH AH0 L OW1}{W ER1 L D}",
    "first {HH AH0 L OW1} middle {W ER1 L D} end.",
    "Tab\tand\nnewline.",
    "Hon. Gen. Maj. Capt. Sgt. Jr. Ltd. Drs.",
    "company broken street",
    "Hello, hello; hello! hello?",
    "a",
    "The way by the world.",
    "Quote \"marks\" and 'single' ones.",
    "Hyphen - alone -- double.",
    "{XX YY} invalid arpabet {HH}.",
    "!",
]


def install_stand_ins():
    def unidecode(text):
        assert text.isascii(), "the capture runs on ASCII sentences only"
        return text

    class Engine:
        def number_to_words(self, *args, **kwargs):
            raise RuntimeError("the capture runs on digit-free sentences only")

    mod = types.ModuleType("unidecode")
    mod.unidecode = unidecode
    sys.modules["unidecode"] = mod
    mod = types.ModuleType("inflect")
    mod.engine = Engine
    sys.modules["inflect"] = mod


def main(reference):
    install_stand_ins()
    sys.path.insert(0, reference)
    from models.parser import CMUDictParser
    assert os.path.realpath(sys.modules["models.parser"].__file__).startswith(os.path.realpath(reference))
    out = {}
    for mode, path in (("chars", None), ("cmudict", os.path.join(HERE, "tiny_cmudict.txt"))):
        parser = CMUDictParser(path)
        out[mode] = {"n_symbols": len(parser.symbols), "symbols": parser.symbols,
                     "cases": [{"text": s, "ids": parser(s)} for s in SENTENCES]}
    if out["cmudict"]:
        d = CMUDictParser(os.path.join(HERE, "tiny_cmudict.txt")).cmu_dict
        out["cmudict"]["entries"] = {w: d.lookup(w) for w in ("hello", "world", "doctor", "'tis", "it's", "the", "way", "by",
                                                               "street", "company", "broken", "absent")}
    with open(os.path.join(HERE, "text_frontend.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: (v["n_symbols"], len(v["cases"])) for k, v in out.items()})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
