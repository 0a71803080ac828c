"""The text front end (models/parser.py) on the CPU: ids and symbol tables against the reference's own parser
(tests/golden/text_frontend.json, written by tests/golden/make_golden_text.py, without a dictionary and with
tests/golden/tiny_cmudict.txt), the number table and the ASCII folding (the parts written without inflect and unidecode),
and what the models and scripts/synthesize.py do with a sentence before anything runs on the device."""
import json
import os
import re

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
TINY_DICT = os.path.join(GOLDEN, "tiny_cmudict.txt")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "text_frontend.json"), encoding="utf-8") as f:
        return json.load(f)


def _parser(mode):
    from models.parser import CMUDictParser
    return CMUDictParser(None if mode == "chars" else TINY_DICT)


@pytest.mark.parametrize("mode,n_symbols", [("chars", 64), ("cmudict", 148)])
def test_ids_and_symbols_equal_the_references(fixture, mode, n_symbols):
    parser, want = _parser(mode), fixture[mode]
    assert len(parser.symbols) == want["n_symbols"] == n_symbols
    assert parser.symbols == want["symbols"]
    assert len(want["cases"]) >= 30
    for case in want["cases"]:
        assert parser(case["text"]) == case["ids"], (mode, case["text"])


def test_fixture_covers_what_it_should(fixture):
    texts = [c["text"] for c in fixture["chars"]["cases"]]
    assert texts == [c["text"] for c in fixture["cmudict"]["cases"]]
    assert all(t.isascii() and not re.search(r"[0-9]", re.sub(r"\{.*?\}", "", t)) for t in texts)   # digits: ARPAbet stress only
    for needle in ("Dr.", "Mr.", "co.", "btw", "www", "  ", "-", "...", "?!"):
        assert any(needle in t for t in texts), needle
    assert any(t.startswith("{") for t in texts) and any(t.endswith("}") for t in texts)
    assert any("{" in t and not t.startswith("{") and not t.endswith("}") for t in texts)
    hello = next(c for c in fixture["chars"]["cases"] if c["text"] == "Hello world.")
    assert hello["ids"] == [45, 42, 49, 49, 52, 11, 60, 52, 55, 49, 41, 7]
    # the two modes really differ: a dictionary word becomes phonemes (ids >= 64)
    hello = next(c for c in fixture["cmudict"]["cases"] if c["text"] == "Hello world.")
    assert max(hello["ids"]) >= 64


def test_dictionary_entries_equal_the_references(fixture):
    from models.parser import CMUDict
    d = CMUDict(TINY_DICT)
    for word, want in fixture["cmudict"]["entries"].items():
        assert d.lookup(word) == want, word
    assert d.lookup("hello") == ["HH AH0 L OW1", "HH EH0 L OW1"]          # WORD(1): the alternate, first one wins in the parser
    assert d.lookup("'tis") == ["T IH1 Z"]                                # an apostrophe word
    assert d.lookup("broken") is None                                     # a symbol outside the table: the line is skipped
    assert len(d) == 10


NUMBERS = [
    ("42", "forty-two"), ("100", "one hundred"), ("101", "one hundred one"), ("1234", "twelve thirty-four"),
    ("1905", "nineteen oh five"), ("1900", "nineteen hundred"), ("2000", "two thousand"), ("2005", "two thousand five"),
    ("3000", "three thousand"), ("12345", "twelve thousand, three hundred forty-five"),
    ("1,234,567", "one million, two hundred thirty-four thousand, five hundred sixty-seven"),
    ("$3.50", "three dollars, fifty cents"), ("$1", "one dollar"), ("$0.05", "five cents"), ("£100", "one hundred pounds"),
    ("3.14", "three point fourteen"), ("2nd", "second"), ("21st", "twenty-first"), ("100th", "one hundredth"),
]


@pytest.mark.parametrize("text,want", NUMBERS)
def test_number_table(text, want):
    parser = _parser("chars")
    assert " ".join(parser.expand_numbers(text).split()) == want
    assert parser.english_cleaners(text).strip() == want                  # the whole cleaning keeps the pound sign for its rule


def test_numbers_inside_a_sentence_reach_the_ids():
    parser = _parser("chars")
    assert parser.sequence_to_text(parser("In 1905 he paid $3.50.")) == "in nineteen oh five he paid three dollars, fifty cents."


def test_ascii_folding():
    from models.parser import fold_to_ascii
    assert fold_to_ascii("café") == "cafe"
    assert fold_to_ascii("“quoted” and ‘single’") == "\"quoted\" and 'single'"
    assert fold_to_ascii("naïve façade Ångström") == "naive facade Angstrom"
    assert fold_to_ascii("a — b … 中") == "a  b ... "          # what is left non-ASCII is dropped; NFKD spells the ellipsis
    parser = _parser("chars")
    assert parser("café") == parser("cafe")


def _glow_config(**dataset):
    from oracle import glow_oracle as go
    from utils import config as C
    return C.create({"model": dict(n_speakers=1, gin_channels=0, encoder=dict(go.GOLDEN_CFG["encoder"], n_vocab=64),
                                   decoder=dict(go.GOLDEN_CFG["decoder"])),
                     "dataset": {**dict(n_mels=8, intersperse_blanks=True, cmudict_path=""), **dataset}})


def test_sentence_ids_strip_period_and_blanks():
    from models.parser import sentence_ids
    parser = _parser("chars")
    ids = sentence_ids(parser, "  Hello world ", True)
    assert ids[1::2] == parser("Hello world.") and set(ids[0::2]) == {64} and len(ids) == 2 * 12 + 1
    assert sentence_ids(parser, "What?", False) == parser("What?")
    for empty in ("", "   \n"):
        with pytest.raises(ValueError, match="empty"):
            sentence_ids(parser, empty, True)

    class Nothing:
        symbols = []

        def __call__(self, text):
            return []

    with pytest.raises(ValueError, match="no symbol"):
        sentence_ids(Nothing(), "~", True)


def test_infer_step_with_and_without_a_front_end():
    from models.glow_tts.glow_tts import GlowTTS
    from models.vqtts.vqtts import VQTTS
    from utils import config as C
    import vqtts_model_helpers as VH
    plain = GlowTTS(_glow_config()).eval()
    assert plain.text_parser is None
    with pytest.raises(NotImplementedError, match="CMUDict"):
        plain.infer_step("hello world.")
    chars = GlowTTS(_glow_config(text_frontend="chars")).eval()
    assert len(chars.text_parser.symbols) == 64 and chars.intersperse_blanks
    for empty in ("", "  "):
        with pytest.raises(ValueError, match="empty"):
            chars.infer_step(empty)
    with pytest.raises(ValueError, match="n_vocab"):                       # 148 symbols do not fit 64 embeddings
        GlowTTS(_glow_config(text_frontend="cmudict", cmudict_path=TINY_DICT))
    missing = os.path.join(GOLDEN, "no_such_cmudict.txt")
    with pytest.raises(ValueError, match="no_such_cmudict.txt"):
        GlowTTS(_glow_config(text_frontend="cmudict", cmudict_path=missing))
    with pytest.raises(ValueError, match="chars or cmudict"):
        GlowTTS(_glow_config(text_frontend="phonemes"))

    cfg = VH.config_dict()
    vq_plain = VQTTS(C.create(cfg)).eval()
    with pytest.raises(NotImplementedError, match="CMUDict"):
        vq_plain.infer_step("hello world.")
    cfg["dataset"]["text_frontend"] = "chars"
    with pytest.raises(ValueError, match="n_vocab"):                       # the helper's 11-id vocabulary
        VQTTS(C.create(cfg))
    cfg["model"]["encoder"]["n_vocab"] = 64
    vq_chars = VQTTS(C.create(cfg)).eval()
    with pytest.raises(ValueError, match="empty"):
        vq_chars.infer_step(" ")
    assert "text_parser" not in "".join(vq_chars.state_dict()) and "text_parser" not in "".join(chars.state_dict())


def test_synthesize_wants_exactly_one_of_tokens_and_text(tmp_path):
    from scripts import synthesize
    base = ["--log_dir", str(tmp_path), "--ckpt_num", "1"]
    with pytest.raises(ValueError, match="exactly one of --tokens .* neither"):
        synthesize.main(base)
    with pytest.raises(ValueError, match="exactly one of --tokens .* both"):
        synthesize.main(base + ["--tokens", "a.txt", "--text", "b.txt"])
    path = tmp_path / "s.txt"
    path.write_text("Hello world.\n\n  second line  \n", encoding="utf-8")
    assert synthesize.read_sentences(str(path)) == ["Hello world.", "second line"]

    class NoFrontEnd:
        text_parser = None

    with pytest.raises(ValueError, match="dataset.text_frontend"):
        synthesize.sentences_to_tokens(NoFrontEnd(), ["hello"], str(path))

    class Chars:
        text_parser, intersperse_blanks = _parser("chars"), True

    got = synthesize.sentences_to_tokens(Chars(), ["Hello world"], str(path))
    assert got[0][1::2] == [45, 42, 49, 49, 52, 11, 60, 52, 55, 49, 41, 7] and got[0][0] == 64
    assert torch.tensor(got[0]).max() == 64
