"""Reader and writer for Praat TextGrid files as Montreal Forced Aligner writes them: the long ("ooTextFile") and the short text format are
read, the long one is written (io_utils/forced_align.py), interval tiers only.  It offers what the reference's importer uses of the `textgrid` package (scripts/import_textgrid.py:249-271): `TextGrid.fromFile(path)`,
`tg[tier][i].mark / .minTime / .maxTime` and `len(tg[tier])`; a tier is addressed by position or by name.

Both formats carry the same values in the same order; the long one only labels them (`xmin = 0`, `intervals [3]:`).  The reader therefore takes
the file as a stream of values — quoted strings (a quote inside a string is doubled), numbers and `<exists>` flags — and skips the labels."""
import re

_VALUE = re.compile(r'"((?:[^"]|"")*)"'                                   # 1: string
                    r'|(<\w+>)'                                           # 2: flag
                    r'|\[[^\]\n]*\]'                                      # an index such as [3]: a label, not a value
                    r'|(?<![\w.])([-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)(?![\w.])')   # 3: number


class Interval:
    __slots__ = ('minTime', 'maxTime', 'mark')

    def __init__(self, minTime, maxTime, mark):
        self.minTime, self.maxTime, self.mark = minTime, maxTime, mark

    def __repr__(self):
        return 'Interval(%r, %r, %r)' % (self.minTime, self.maxTime, self.mark)


class IntervalTier:
    def __init__(self, name, minTime, maxTime, intervals):
        self.name, self.minTime, self.maxTime, self.intervals = name, minTime, maxTime, intervals

    def __len__(self):
        return len(self.intervals)

    def __getitem__(self, i):
        return self.intervals[i]

    def __iter__(self):
        return iter(self.intervals)


def _decode(raw):
    if raw[:2] in (b'\xff\xfe', b'\xfe\xff'):
        return raw.decode('utf-16')
    if raw[:3] == b'\xef\xbb\xbf':
        return raw[3:].decode('utf-8')
    return raw.decode('utf-8')


class _Values:
    def __init__(self, text, where):
        self._it = _VALUE.finditer(text)
        self._where = where

    def _next(self, group, what):
        for m in self._it:
            if m.group(1) is None and m.group(2) is None and m.group(3) is None:
                continue                                   # a bracketed index
            if m.group(group) is None:
                raise ValueError('%s: expected %s, found %r' % (self._where, what, m.group(0)))
            return m.group(group)
        raise ValueError('%s: the file ends where %s should be' % (self._where, what))

    def string(self, what):
        return self._next(1, what).replace('""', '"')

    def number(self, what):
        return float(self._next(3, what))

    def count(self, what):
        v = self.number(what)
        if v < 0 or v != int(v):
            raise ValueError('%s: %s is %r' % (self._where, what, v))
        return int(v)

    def flag(self, what):
        return self._next(2, what)


class TextGrid:
    def __init__(self, minTime=0.0, maxTime=0.0, tiers=None):
        self.minTime, self.maxTime, self.tiers = minTime, maxTime, list(tiers or [])

    def __len__(self):
        return len(self.tiers)

    def __iter__(self):
        return iter(self.tiers)

    def __getitem__(self, key):
        if isinstance(key, str):
            for tier in self.tiers:
                if tier.name == key:
                    return tier
            raise KeyError(key)
        return self.tiers[key]

    @classmethod
    def fromFile(cls, path):
        with open(path, 'rb') as f:
            return cls.fromString(_decode(f.read()), where=str(path))

    @classmethod
    def fromString(cls, text, where='<string>'):
        text = '\n'.join(line for line in text.splitlines() if not line.lstrip().startswith('!'))    # (Praat's comment lines)
        v = _Values(text, where)
        if v.string('the file type') != 'ooTextFile' or v.string('the object class') != 'TextGrid':
            raise ValueError('%s: not a Praat TextGrid text file' % where)
        tg = cls(v.number('xmin'), v.number('xmax'))
        if v.flag('the tiers flag') != '<exists>':
            return tg
        for _ in range(v.count('the number of tiers')):
            kind, name = v.string('a tier class'), v.string('a tier name')
            if kind != 'IntervalTier':
                raise ValueError('%s: tier %r is a %s; only interval tiers are read (point tiers carry no durations)' % (where, name, kind))
            lo, hi = v.number('xmin'), v.number('xmax')
            items = []
            for _ in range(v.count('the number of intervals')):
                a, b = v.number('xmin'), v.number('xmax')
                items.append(Interval(a, b, v.string('an interval text')))
            tg.tiers.append(IntervalTier(name, lo, hi, items))
        return tg

    def toString(self):
        """the long text format; numbers are written with repr, so that fromString returns the same floats"""
        q = lambda text: '"' + str(text).replace('"', '""') + '"'
        out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', '', 'xmin = %r' % float(self.minTime), 'xmax = %r' % float(self.maxTime),
               'tiers? <exists>', 'size = %d' % len(self.tiers), 'item []:']
        for k, tier in enumerate(self.tiers):
            out += ['    item [%d]:' % (k + 1), '        class = "IntervalTier"', '        name = %s' % q(tier.name),
                    '        xmin = %r' % float(tier.minTime), '        xmax = %r' % float(tier.maxTime),
                    '        intervals: size = %d' % len(tier.intervals)]
            for i, iv in enumerate(tier.intervals):
                out += ['        intervals [%d]:' % (i + 1), '            xmin = %r' % float(iv.minTime), '            xmax = %r' % float(iv.maxTime),
                        '            text = %s' % q(iv.mark)]
        return '\n'.join(out) + '\n'

    def write(self, path):
        with open(path, 'w', encoding='utf-8', newline='\n') as f:
            f.write(self.toString())
