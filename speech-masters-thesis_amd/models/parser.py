"""Text front end of the token models (reference models/parser.py): ``CMUDictParser`` turns a sentence into symbol ids --
characters, or ARPAbet phonemes for the words a CMU pronouncing dictionary knows -- and ``CMUDict`` reads that dictionary.

Ids, symbol order and ``len(symbols)`` are the reference's (64 symbols without a dictionary, 148 with one): the pad ``_``, the
hyphen, ``!'(),.:;? ``, A-Z, a-z, then the 84 ARPAbet symbols with an ``@`` in front.  tests/golden/text_frontend.json pins
them against the reference's own parser, in both modes.

Kept from the reference, quirks included:
  * cleaning = ASCII folding, lower case, number expansion, abbreviations and replacements, whitespace collapse, in this order;
  * ``{HH AH0 L OW1}`` holds ARPAbet; the text BEFORE a curly group is spelled in characters even with a dictionary, and only
    the text after the last group is looked up word by word (``[\\w']+|[.,!?;]``: other punctuation is dropped there);
  * with a dictionary every word or mark is followed by a space and the trailing one is removed; the first pronunciation wins;
  * a symbol outside the table is dropped silently (in character mode that is every ARPAbet symbol of a curly group).

Written without ``unidecode`` and ``inflect`` (DESIGN.md section 18 lists the deviations):
  * ASCII folding is NFKD with the combining marks dropped, curly quotes mapped to ``'`` and ``"``; whatever else stays
    non-ASCII is dropped, except the pound sign, which is kept for the pounds rule of the number expansion;
  * numbers are spelled by ``number_to_words`` / ``ordinal_to_words`` below, which cover what the reference asks of inflect:
    cardinals without "and", ordinals, and the two-digit grouping of the 1000-3000 "year" rule.
"""
import os
import re
import unicodedata
from typing import List, Optional

VALID_SYMBOLS = [
    "AA", "AA0", "AA1", "AA2", "AE", "AE0", "AE1", "AE2", "AH", "AH0", "AH1", "AH2", "AO", "AO0", "AO1", "AO2", "AW",
    "AW0", "AW1", "AW2", "AY", "AY0", "AY1", "AY2", "B", "CH", "D", "DH", "EH", "EH0", "EH1", "EH2", "ER", "ER0",
    "ER1", "ER2", "EY", "EY0", "EY1", "EY2", "F", "G", "HH", "IH", "IH0", "IH1", "IH2", "IY", "IY0", "IY1", "IY2",
    "JH", "K", "L", "M", "N", "NG", "OW", "OW0", "OW1", "OW2", "OY", "OY0", "OY1", "OY2", "P", "R", "S", "SH", "T",
    "TH", "UH", "UH0", "UH1", "UH2", "UW", "UW0", "UW1", "UW2", "V", "W", "Y", "Z", "ZH",
]

_ONES = ["zero", "one", "two", "three", "four", "five", "six", "seven", "eight", "nine", "ten", "eleven", "twelve",
         "thirteen", "fourteen", "fifteen", "sixteen", "seventeen", "eighteen", "nineteen"]
_TENS = ["", "", "twenty", "thirty", "forty", "fifty", "sixty", "seventy", "eighty", "ninety"]
_SCALES = ["", "thousand", "million", "billion", "trillion", "quadrillion", "quintillion", "sextillion", "septillion",
           "octillion", "nonillion", "decillion"]
_ORDINALS = {"one": "first", "two": "second", "three": "third", "five": "fifth", "eight": "eighth", "nine": "ninth",
             "twelve": "twelfth"}


def _below_hundred(n):
    return _ONES[n] if n < 20 else _TENS[n // 10] + ("-" + _ONES[n % 10] if n % 10 else "")


def _below_thousand(n, andword):
    hundreds, rest = divmod(n, 100)
    words = [_ONES[hundreds], "hundred"] if hundreds else []
    if rest:
        if hundreds and andword:
            words.append(andword)
        words.append(_below_hundred(rest))
    return " ".join(words)


def number_to_words(num: int, andword: str = "") -> str:
    """Cardinal in words: thousands groups joined by ", " ("twelve thousand, three hundred forty-five").  A last group below one
    hundred is one word, and joins with `andword` instead of the comma ("five thousand one"; "one thousand and one").  A number
    of more than 36 digits is spelled digit by digit."""
    if num == 0:
        return "zero"
    if num >= 10 ** (3 * len(_SCALES)):
        return " ".join(_ONES[int(d)] for d in str(num))
    groups, scale = [], 0
    while num:
        num, g = divmod(num, 1000)
        if g:
            groups.append((g, scale))
        scale += 1
    chunks = [_below_thousand(g, andword) + (" " + _SCALES[s] if s else "") for g, s in reversed(groups)]
    if len(chunks) > 1 and groups[0][1] == 0 and groups[0][0] < 100:
        return ", ".join(chunks[:-1]) + (" " + andword if andword else "") + " " + chunks[-1]
    return ", ".join(chunks)


def ordinal_to_words(num: int) -> str:
    """Ordinal in words ("twenty-first", "one hundredth", "one hundred and first"): the cardinal with "and", last word turned."""
    words = number_to_words(num, andword="and")
    cut = max(words.rfind(" "), words.rfind("-")) + 1
    head, last = words[:cut], words[cut:]
    if last in _ORDINALS:
        last = _ORDINALS[last]
    elif last.endswith("y"):
        last = last[:-1] + "ieth"
    else:
        last += "th"
    return head + last


def year_to_words(num: int) -> str:
    """Digits read in pairs from the left, a leading zero as "oh": 1905 -> "nineteen oh five", 1234 -> "twelve thirty-four"."""
    digits = str(num)
    pairs = [digits[i:i + 2] for i in range(0, len(digits), 2)]
    return " ".join("oh " + _ONES[int(p[1])] if len(p) == 2 and p[0] == "0" else _below_hundred(int(p)) for p in pairs)


_QUOTES = {"‘": "'", "’": "'", "‚": "'", "‛": "'", "“": '"', "”": '"', "„": '"',
           "‟": '"'}


def fold_to_ascii(text: str) -> str:
    out = []
    for ch in unicodedata.normalize("NFKD", "".join(_QUOTES.get(c, c) for c in text)):
        if ch < "\x80" or ch == "£":
            out.append(ch)
    return "".join(out)


class CMUDict(object):
    """word -> list of ARPAbet pronunciations, read from a CMU pronouncing dictionary (two spaces between word and phonemes,
    ``WORD(1)`` for an alternate, ``;;;`` comments).  Lines that do not start with A-Z or an apostrophe, and pronunciations with
    a symbol outside the 84 valid ones, are skipped."""

    def __init__(self, file_or_path, keep_ambiguous=True):
        self.valid_symbols = list(VALID_SYMBOLS)
        self._valid = set(self.valid_symbols)
        if isinstance(file_or_path, str):
            with open(file_or_path, encoding="latin-1") as f:
                entries = self._parse(f)
        else:
            entries = self._parse(file_or_path)
        if not keep_ambiguous:
            entries = {word: pron for word, pron in entries.items() if len(pron) == 1}
        self._entries = entries

    def __len__(self):
        return len(self._entries)

    def lookup(self, word):
        """ARPAbet pronunciations of `word` (any case), or None."""
        return self._entries.get(word.upper())

    def _parse(self, lines):
        alt = re.compile(r"\([0-9]+\)")
        entries = {}
        for line in lines:
            if not line or not ("A" <= line[0] <= "Z" or line[0] == "'"):
                continue
            parts = line.split("  ")
            if len(parts) < 2:
                continue
            phonemes = parts[1].strip().split(" ")
            if all(p in self._valid for p in phonemes):
                entries.setdefault(alt.sub("", parts[0]), []).append(" ".join(phonemes))
        return entries


_ABBREVIATIONS = [("mrs", "missus"), ("mr", "mister"), ("dr", "doctor"), ("st", "saint"), ("co", "company"), ("jr", "junior"),
                  ("maj", "major"), ("gen", "general"), ("drs", "doctors"), ("rev", "reverend"), ("lt", "lieutenant"),
                  ("hon", "honorable"), ("sgt", "sergeant"), ("capt", "captain"), ("esq", "esquire"), ("ltd", "limited"),
                  ("col", "colonel"), ("ft", "fort")]
_REPLACEMENTS = [("_", "underscore"), ("src", "source"), ("dll", "d l l"), ("btw", "by the way"), ("http", "h t t p"),
                 ("www", "w w w"), (r"c\+\+", "c plus plus")]


class CMUDictParser(object):

    def __init__(self, cmu_dict_path=None):
        self.cmu_dict = CMUDict(cmu_dict_path) if cmu_dict_path else None
        self.symbols = ["_", "-"] + list("!'(),.:;? ") + list("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")
        if self.cmu_dict:
            self.symbols = self.symbols + ["@" + s for s in self.cmu_dict.valid_symbols]   # "@": some equal capital letters
        self._symbol_to_id = {s: i for i, s in enumerate(self.symbols)}
        self._id_to_symbol = dict(enumerate(self.symbols))
        self._curly_re = re.compile(r"(.*?)\{(.+?)\}(.*)")
        self._abbreviations = [(re.compile(r"\b%s\." % a, re.IGNORECASE), b) for a, b in _ABBREVIATIONS]
        self._replacements = [(re.compile(r"\b%s\b" % a, re.IGNORECASE), b) for a, b in _REPLACEMENTS]

    def __call__(self, text: str) -> Optional[List[int]]:
        return self.text_to_sequence(text)

    # ------------------------------------------------------------------------------------------------ cleaning
    def _expand_dollars(self, m):
        parts = m.group(1).split(".")
        if len(parts) > 2:
            return m.group(1) + " dollars"
        dollars = int(parts[0]) if parts[0] else 0
        cents = int(parts[1]) if len(parts) > 1 and parts[1] else 0
        d = "%d %s" % (dollars, "dollar" if dollars == 1 else "dollars")
        c = "%d %s" % (cents, "cent" if cents == 1 else "cents")
        if dollars and cents:
            return d + ", " + c
        return d if dollars else c if cents else "zero dollars"

    @staticmethod
    def _expand_number(m):
        num = int(m.group(0))
        if 1000 < num < 3000:
            if num == 2000:
                return "two thousand"
            if 2000 < num < 2010:
                return "two thousand " + number_to_words(num % 100)
            if num % 100 == 0:
                return number_to_words(num // 100) + " hundred"
            return year_to_words(num)
        return number_to_words(num)

    def expand_numbers(self, text):
        """Commas out of numbers, pounds, dollars, the decimal point, ordinals, digit runs split off, cardinals -- in this
        order.  The split leaves a space on both sides of every number; `english_cleaners` collapses the runs afterwards."""
        text = re.sub(r"([0-9][0-9,]+[0-9])", lambda m: m.group(1).replace(",", ""), text)
        text = re.sub("£([0-9,]*[0-9]+)", r"\1 pounds", text)
        text = re.sub(r"\$([0-9.,]*[0-9]+)", self._expand_dollars, text)
        text = re.sub(r"([0-9]+\.[0-9]+)", lambda m: m.group(1).replace(".", " point "), text)
        text = re.sub(r"([0-9]+)(st|nd|rd|th)", lambda m: ordinal_to_words(int(m.group(1))), text)
        text = " ".join(re.split(r"(\d+)", text))
        return re.sub(r"[0-9]+", self._expand_number, text)

    def replace(self, text):
        for regex, replacement in self._abbreviations + self._replacements:
            text = regex.sub(replacement, text)
        return text

    def english_cleaners(self, text):
        text = fold_to_ascii(text).lower()
        text = self.replace(self.expand_numbers(text))
        return re.sub(r"\s+", " ", text)

    # ------------------------------------------------------------------------------------------------ symbols
    def _symbols_to_sequence(self, symbols):
        return [self._symbol_to_id[s] for s in symbols if s in self._symbol_to_id and s != "_" and s != "~"]

    def _arpabet_to_sequence(self, text):
        return self._symbols_to_sequence(["@" + s for s in text.split()])

    def text_to_sequence(self, text):
        """Sentence -> ids.  ``{...}`` groups hold ARPAbet (see the module docstring for what happens around them)."""
        sequence = []
        space = self._symbols_to_sequence(" ")
        while len(text):
            m = self._curly_re.match(text)
            if not m:
                clean = self.english_cleaners(text)
                if self.cmu_dict is None:
                    sequence += self._symbols_to_sequence(clean)
                else:
                    for word in re.findall(r"[\w']+|[.,!?;]", clean):
                        pron = self.cmu_dict.lookup(word)
                        sequence += self._arpabet_to_sequence(pron[0]) if pron is not None else self._symbols_to_sequence(word)
                        sequence += space
                break
            sequence += self._symbols_to_sequence(self.english_cleaners(m.group(1)))
            sequence += self._arpabet_to_sequence(m.group(2))
            text = m.group(3)
        if self.cmu_dict is not None and sequence and sequence[-1] == space[0]:
            sequence = sequence[:-1]
        return sequence

    def sequence_to_text(self, sequence):
        """Ids back to a string, ARPAbet in curly braces."""
        result = ""
        for symbol_id in sequence:
            s = self._id_to_symbol.get(symbol_id)
            if s is not None:
                result += "{%s}" % s[1:] if len(s) > 1 and s[0] == "@" else s
        return result.replace("}{", " ")


def parser_from_config(dataset_config):
    """The parser `dataset.text_frontend` names: "chars" (no dictionary, 64 symbols) or "cmudict" (the dictionary at
    `dataset.cmudict_path`, 148 symbols); None when the key is unset.  ValueError, naming the path, when the dictionary is
    asked for and its file does not exist."""
    frontend = dataset_config.get("text_frontend")
    if not frontend:
        return None
    if frontend == "chars":
        return CMUDictParser(None)
    if frontend == "cmudict":
        path = dataset_config.get("cmudict_path")
        if not path or not os.path.isfile(path):
            raise ValueError(f"dataset.text_frontend = cmudict needs the CMU pronouncing dictionary: dataset.cmudict_path = {path!r} "
                             "is not a file (dataset.text_frontend = chars needs none)")
        return CMUDictParser(path)
    raise ValueError(f"dataset.text_frontend must be chars or cmudict, got {frontend!r}")


def blank_interspersed(token, blank):
    """[blank, t0, blank, t1, ..., blank]: 2 n + 1 ids (reference datasets/ljspeech.py:100-103)."""
    out = [blank] * (2 * len(token) + 1)
    out[1::2] = token
    return out


def sentence_ids(parser, text, intersperse_blanks):
    """What the dataset does to a transcript and `infer_step` to a sentence: strip, append "." unless it ends in . ! ?, parse,
    intersperse the blank id len(parser.symbols).  ValueError for a text that is empty or leaves no symbol."""
    text = text.strip()
    if not text:
        raise ValueError("the text is empty")
    if text[-1] not in ".!?":
        text += "."
    token = parser(text)
    if not token:
        raise ValueError(f"no symbol of the text {text!r} is in the parser's table")
    return blank_interspersed(token, len(parser.symbols)) if intersperse_blanks else token
