"""What the tests of ZKGPU_TXFORMAT_RETURN_LOG share: a log record taken apart, and the two checks that pin its contents
with nothing but the oracle's Merlin transcript (oracle.binding.MerlinTranscript):

  the transaction ID is the Merkle root over [header, entries] (oracle/zkvm_tx.c; UNPINNED row tx.txid.tree), so the root
  recomputed from a returned record must be the oracle's transaction ID -- a wrong ID, order, kind or count changes it;
  an input's ID is the contract ID of the serialized contract the program pushed before its `input` opcode.
"""
INPUT, OUTPUT = 1, 2
NAMES = {INPUT: "input", OUTPUT: "output"}


def record_bytes(k):
    return 1 + 33 * k


def area_bytes(batch, k):
    """bytes of the status argument of a call of `batch` transactions under the flag with window k"""
    return batch * (33 + record_bytes(k))


def split_area(raw, batch, k):
    """the status argument of a flagged call -> (status bytes, [ids], [records])"""
    per = record_bytes(k)
    return (raw[:batch], [raw[batch + 32 * i: batch + 32 * i + 32] for i in range(batch)],
            [raw[33 * batch + per * i: 33 * batch + per * (i + 1)] for i in range(batch)])


def parse_record(rec, k):
    """-> (count, [(kind, id)] for the entries the record holds); asserts that everything past them is zero"""
    assert len(rec) == record_bytes(k)
    count = rec[0]
    held = count if count <= k else 0
    kinds, ids = rec[1: 1 + k], rec[1 + k:]
    assert kinds[held:] == bytes(k - held) and ids[32 * held:] == bytes(32 * (k - held)), "bytes past the entries are not zero"
    return count, [(kinds[j], ids[32 * j: 32 * j + 32]) for j in range(held)]


def _leaf(oracle, entry):
    t = oracle.MerlinTranscript(b"ZkVM.txid")
    if entry[0] == "header":
        t.append_u64(b"tx.version", entry[1])
        t.append_u64(b"tx.mintime", entry[2])
        t.append_u64(b"tx.maxtime", entry[3])
    else:
        t.append_message(NAMES[entry[0]].encode(), entry[1])
    return t.challenge_bytes(b"merkle.leaf", 32)


def _root(oracle, leaves):
    if len(leaves) == 1:
        return leaves[0]
    k = 1
    while 2 * k < len(leaves):
        k *= 2
    t = oracle.MerlinTranscript(b"ZkVM.txid")
    t.append_message(b"L", _root(oracle, leaves[:k]))
    t.append_message(b"R", _root(oracle, leaves[k:]))
    return t.challenge_bytes(b"merkle.node", 32)


def merkle_root(oracle, tx, entries):
    """the transaction ID that follows from the transaction's header and the (kind, id) entries of a record"""
    header = ("header",) + tuple(int.from_bytes(tx[8 * q: 8 * q + 8], "little") for q in range(3))
    return _root(oracle, [_leaf(oracle, header)] + [_leaf(oracle, e) for e in entries])


def input_contracts(tx):
    """the serialized contracts a payment's program pushes right before each of its `input` opcodes, in order"""
    n = int.from_bytes(tx[24:28], "little")
    prog, pc, last, out = tx[28: 28 + n], 0, None, []
    width = {0x02: 0, 0x03: 4, 0x04: 4, 0x06: 0, 0x18: 8, 0x1c: 4, 0x20: 0}
    while pc < len(prog):
        op = prog[pc]
        pc += 1
        if op == 0x00:
            ln = int.from_bytes(prog[pc: pc + 4], "little")
            last = prog[pc + 4: pc + 4 + ln]
            pc += 4 + ln
            continue
        if op == 0x1b:
            assert last is not None, "an input that does not follow a push"
            out.append(last)
        else:
            pc += width[op]
        last = None
    return out


def contract_id(oracle, contract):
    t = oracle.MerlinTranscript(b"ZkVM.contractid")
    t.append_message(b"contract", contract)
    return t.challenge_bytes(b"id", 32)


def check_accepted(oracle, tx, txid, rec, k):
    """a record beside an accepted transaction: fits the window -> its entries reproduce the oracle's transaction ID and the
    returned one, and its inputs are the contract IDs of the pushed contracts; does not fit -> the real count and zeros.
    -> the count"""
    rc, want, _, _ = oracle.tx_id(tx)
    assert rc == 0 and txid == want
    contracts = input_contracts(tx)
    n_out = sum(1 for q in _opcodes(tx) if q == 0x1c)
    count, entries = parse_record(rec, k)
    assert count == len(contracts) + n_out
    if count > k:
        assert entries == []
        return count
    assert merkle_root(oracle, tx, entries) == want, "the record's entries do not hash to the transaction ID"
    assert [i for kind, i in entries if kind == INPUT] == [contract_id(oracle, c) for c in contracts]
    assert len([1 for kind, _ in entries if kind == OUTPUT]) == n_out
    return count


def _opcodes(tx):
    n = int.from_bytes(tx[24:28], "little")
    prog, pc = tx[28: 28 + n], 0
    width = {0x02: 0, 0x03: 4, 0x04: 4, 0x06: 0, 0x18: 8, 0x1b: 0, 0x1c: 4, 0x20: 0}
    while pc < len(prog):
        op = prog[pc]
        pc += 1
        if op == 0x00:
            pc += 4 + int.from_bytes(prog[pc: pc + 4], "little")
        else:
            pc += width[op]
        yield op
