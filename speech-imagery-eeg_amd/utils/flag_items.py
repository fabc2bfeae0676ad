"""The item loop of the four ``--eeg_*`` flags, and (``parse_spec``) the whole parser of ``--faithfulness`` and ``--occlusion``: a comma
list of ``key=value`` items and bare keys, one grammar per flag.  ``FlagItems``
splits the text, refuses unknown and repeated keys and converts numbers, and words every refusal as that flag always has; what a
value means (a band, a ratio, a file) stays with the flag's own parser.  No numpy and no torch in this module."""
import math


class FlagItems:
    """`keys`: every key of the flag; `bare`: those that stand without ``=`` (``fit``, ``envelope``); `need_value`: an empty value
    behind ``=`` is refused here (else the flag's parser words it); `expected`: refusals other than "is not one of" end with
    ``; expected <grammar>``; `strip_value`: False hands the value on as typed, for a flag whose refusals quote it so."""

    def __init__(self, flag, grammar, keys, bare=(), need_value=True, expected=True, strip_value=True):
        self.flag, self.grammar, self.keys, self.bare, self.need_value = flag, grammar, tuple(keys), tuple(bare), bool(need_value)
        self.strip_value = bool(strip_value)
        self.tail = f"; expected {grammar}" if expected else ""

    def clean(self, text):
        """None / '' / 'none' (any case) -> None: the flag is off; else the stripped text"""
        text = '' if text is None else str(text).strip()
        return None if text.lower() in ('', 'none') else text

    def items(self, text):
        """(key, value) per item, in the order given ('' for a bare key); the caller converts inside the loop, so the first
        refusal is the left-most item's"""
        seen = set()
        for item in text.split(','):
            key, eq, val = item.partition('=')
            key, val = key.strip(), val.strip() if self.strip_value else val
            if key not in self.keys or (key in self.bare) == bool(eq) or (self.need_value and eq and not val):
                raise ValueError(f"{self.flag}: {item!r} is not one of {self.grammar}")
            if key in seen:
                raise ValueError(f"{self.flag}: {key} given twice{self.tail}")
            seen.add(key)
            yield key, val

    def number(self, key, val, finite=True):
        try:
            out = float(val)
        except ValueError:
            raise ValueError(f"{self.flag}: {key}={val!r} is not a number{self.tail}") from None
        if finite and not math.isfinite(out):
            raise ValueError(f"{self.flag}: {key}={val!r} is not finite{self.tail}")
        return out

    def integer(self, key, val):
        try:
            return int(val)
        except ValueError:
            raise ValueError(f"{self.flag}: {key}={val!r} is not an integer{self.tail}") from None


def parse_spec(items, spec, cls, check, required, integers=(), convert=None):
    """A flag whose items are the fields of the NamedTuple `cls` (--faithfulness, --occlusion): ``none`` / ``''`` / None -> None (the
    flag is off), a `cls` -> itself, else the ``key=value`` list -> `cls`, checked by ``check(*fields)``.  `items`: the flag's
    FlagItems; `integers`: the keys converted with ``items.integer``; `convert`: key -> (field, converter) for a value that lands in
    another field; `required`: ``key=what|it|takes``, the item that must be given, as the refusal words it."""
    if isinstance(spec, cls):
        return spec
    text = items.clean(spec)
    if text is None:
        return None
    got = {}
    for key, val in items.items(text):
        if key in integers:
            got[key] = items.integer(key, val)
        else:
            field, fn = (convert or {}).get(key, (key, str))
            got[field] = fn(val)
    if required.partition('=')[0] not in got:
        raise ValueError(f"{items.flag}: {text!r} names no {required}{items.tail}")
    out = cls(**got)
    check(*out)
    return out
