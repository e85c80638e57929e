"""The case table of tests/stream_order.py covers include/rcu.h: every entry point that takes a stream has a row (or an exemption with a reason), and
every host array such an entry point reads is one the protocol scribbles over after the call.  No device."""
import os
import re

import stream_order as so

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rcu.h')


def prototypes(text):
    """[(name, [parameter declarations])] of every function the header declares."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'^\s*#.*$', '', text, flags=re.M)
    out = []
    for name, args in re.findall(r'\b(rcu_\w+)\s*\(([^;{}()]*)\)\s*;', text):
        out.append((name, [' '.join(a.split()) for a in args.split(',')]))
    return out


def stream_entry_points(text):
    """name -> names of its ``*_host`` parameters, for the functions with a ``void* stream`` parameter."""
    found = {}
    for name, params in prototypes(text):
        if any(re.fullmatch(r'void\s*\*\s*stream', p) for p in params):
            found[name] = [re.search(r'(\w+)$', p).group(1) for p in params if re.search(r'\w+_host$', p)]
    return found


def header():
    with open(HEADER) as f:
        return f.read()


def check_table(text, cases, exempt):
    """What the table owes the header; raises AssertionError naming the difference."""
    entry_points = stream_entry_points(text)
    rows, spared = set(cases), set(exempt)
    assert not rows & spared, 'both a row and an exemption: {}'.format(sorted(rows & spared))
    missing, stale = set(entry_points) - rows - spared, (rows | spared) - set(entry_points)
    assert not missing, 'stream-taking entry points without a row in stream_order.CASES: {}'.format(sorted(missing))
    assert not stale, 'rows for functions include/rcu.h does not declare with a stream: {}'.format(sorted(stale))
    for name, hosts in entry_points.items():
        if name in cases:
            assert set(hosts) <= set(cases[name].hosts), '{}: host arrays {} are not scribbled over'.format(name, sorted(set(hosts) - set(cases[name].hosts)))


def test_the_parser_reads_the_header():
    found = stream_entry_points(header())
    assert len(found) >= 55, sorted(found)
    assert found['rcu_softmax'] == [] and found['rcu_key_hist'] == ['prefixes_host']
    assert found['rcu_dropout_masks'] == ['seeds_host', 'site_channels_host', 'site_keep_host']
    assert 'rcu_unet_create' not in found and 'rcu_ece_thresholds' not in found and 'rcu_unet_profile_begin' not in found


def test_every_stream_taking_entry_point_has_a_row():
    check_table(header(), so.CASES, so.EXEMPT)


def test_reasons_are_given():
    for table in (so.EXEMPT, so.BLOCKS_THE_HOST):
        for name, reason in table.items():
            assert isinstance(reason, str) and reason.strip(), name
    assert set(so.BLOCKS_THE_HOST) <= set(so.CASES)


def test_every_row_has_variants():
    for name, case in so.CASES.items():
        assert len(case.variants) >= 1 and callable(case.build), name


def test_a_deleted_row_is_noticed():
    cases = dict(so.CASES)
    del cases['rcu_softmax']
    try:
        check_table(header(), cases, so.EXEMPT)
    except AssertionError as e:
        assert 'rcu_softmax' in str(e)
    else:
        raise AssertionError('a missing row went unnoticed')


def test_a_new_prototype_is_noticed():
    added = header().replace('#ifdef __cplusplus\n}', 'int rcu_new_thing(const float* x_dev, const int32_t* table_host, size_t n,\n'
                             '                  void* stream);\n#ifdef __cplusplus\n}', 1)
    assert added != header()
    try:
        check_table(added, so.CASES, so.EXEMPT)
    except AssertionError as e:
        assert 'rcu_new_thing' in str(e)
    else:
        raise AssertionError('a new stream-taking prototype went unnoticed')


def test_an_unscribbled_host_array_is_noticed():
    cases = dict(so.CASES)
    cases['rcu_key_hist'] = so.Case(cases['rcu_key_hist'].build, cases['rcu_key_hist'].variants, ())
    try:
        check_table(header(), cases, so.EXEMPT)
    except AssertionError as e:
        assert 'prefixes_host' in str(e)
    else:
        raise AssertionError('a host array nobody scribbles over went unnoticed')
