// bnz_main.cpp -- `bnzhip`: command-line front end over libbzhip.so with the interface of the reference's `bnz` (reference
// bnz/src/main.rs:32-59 usage, :173-257 argument grammar, :259-285 I/O plumbing, :11-14 exit codes).  No compression, decoding or
// matching logic lives here.  A map of the file, top to bottom ("The CLI's shape": where a new option and a new mode go):
//   usage()       the text of --help
//   Options       everything the argument loop decides, as plain fields, and the Mode that check() chooses
//   OPTS, parse() the grammar: one row an option (names, whether it clusters, its value, its "requires" message), read by that table alone;
//                 apply() and take_value() hold what each option sets
//   check()       the cross-option checks, one a line, in the order that decides which of two errors is reported; it leaves the strings
//                 un-hexed or escaped, `regex` decided, `look` filled and the Mode chosen
//   Device        the context and the optional pattern set: opened from $BZHIP_DEVICE, one fail(), one close(); with_retry() beside it
//   files         read_all, read_input, regular_size, read_span, output_of / open_output, finish_input, write_index, load_index
//   run_*()       one function a mode; search, grep and match take the loaded SearchInput and hold their four-way call (set? x indexed?)
//                 once, apart from their printing.  main(): parse, check, switch on the Mode
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cerrno>
#include <cstring>
#include <sys/stat.h>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/bzhip.h"

namespace {
const int SUCCESS = 0, ERR_ARGS = 1, ERR_FILESYSTEM = 2, ERR_OUTPUT = 3; // bnz/src/main.rs:11-14
const int LOST_BLOCKS = 4; // --recover: the salvage is written, blocks were lost (no counterpart in the reference)
const char *TAGLINE = "bnzhip: bzip2 encoder with banzai's output, computed on an AMD MI355X";
const char *VERSION = "version alpha 0.3.1-hip";
const size_t CHUNK = (size_t)16 << 20; // one read of the input; the first room of the bytes a grep or a match writes
const size_t ENTRIES = (size_t)1 << 16; // the first room of hits, lines and matches
const uint8_t NOTHING = 0;              // what an empty input points at

[[noreturn]] void die(int code, const std::string &msg)
{
    fprintf(stderr, "%s\n", msg.c_str());
    exit(code);
}

// a whole stream -> memory, in reads of CHUNK; false: the read failed
bool read_all(FILE *f, std::vector<uint8_t> &data)
{
    std::unique_ptr<uint8_t[]> buf(new uint8_t[CHUNK]);
    for (;;) {
        const size_t k = fread(buf.get(), 1, CHUNK, f);
        data.insert(data.end(), buf.get(), buf.get() + k);
        if (k < CHUNK) return !ferror(f);
    }
}
FILE *open_file(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + path + ": " + strerror(errno));
    return f;
}

[[noreturn]] void usage(bool full)
{
    fprintf(stderr, "%s\n", TAGLINE);
    if (!full) {
        fprintf(stderr, "   run 'bnzhip --help' for a full list of options\n");
        fprintf(stderr, "   run 'bnzhip --info' for information about this software\n%s\n", VERSION);
        exit(ERR_ARGS);
    }
    fprintf(stderr,
            "\n  usage: bnzhip [options] <input_path>\n\n"
            "  options:\n"
            "     --output <path.bz2>    write the stream to this file\n"
            "     --stdout    or   -c    write the stream to standard out\n"
            "     --decompress or  -d    decode <input_path> (one or more .bz2 streams) instead\n"
            "     --stream               with -d: decode in fixed-size buffers, writing as bytes arrive\n"
            "     --recover              decode every block of a damaged <input_path> that still verifies\n"
            "     --index <path>         compressing: also write the index of the stream to <path>;\n"
            "                            with -d and --range: the index of <input_path> to read by\n"
            "     --interval <n>         with --index while compressing, or --make-index: a sync point every <n>\n"
            "                            groups of 50 symbols inside each block (default 256; 0: blocks only)\n"
            "     --make-index <path>    write the index of <input_path> (a .bz2) to <path>; nothing is decoded\n"
            "                            to an output, and the input is kept\n"
            "     --range <off>:<len>    with -d --index: write only these bytes of the decoded data; may repeat\n"
            "     --search <string>      print 'offset<TAB>line' of every occurrence of <string> (1 to 256 bytes) in the\n"
            "                            decoded data, lines counted from 0 by '\\n'; nothing is written, the input is kept\n"
            "     --grep <string>        write the lines of the decoded data that hold <string> (1 to 256 bytes) to standard\n"
            "                            out as they are, selected on the GPU; the input is kept\n"
            "     --invert               with --grep: the lines that do not hold <string>\n"
            "     --line-number          with --grep: prefix each line with its number, from 1, and ':' ('-' on a context line)\n"
            "  -o --only-matching        with --grep: write the matched parts alone, each on a line of its own: the matches\n"
            "                            that do not overlap, leftmost first and the longest there, selected and compacted\n"
            "                            on the device (bzh_match); --count still counts lines; not with --invert, -A, -B, -C\n"
            "  -b --byte-offset          with --grep: prefix each line with the offset of its first byte in the decoded data\n"
            "                            and ':' ('-' on a context line), behind the line number; with -o: of each match\n"
            "  -A --after-context <n>    with --grep: also write the <n> lines behind every selected line,\n"
            "  -B --before-context <n>   ... the <n> lines in front of it,\n"
            "  -C --context <n>          ... or both; every line once and in order, chosen on the device in the same pass,\n"
            "                            a line '--' between two groups of lines that are not adjacent; --count still\n"
            "                            prints the selected lines alone\n"
            "     --grep <string> <input_path> <input_path> ...\n"
            "                            several inputs, with --grep only: every file's selected lines as 'name:line'\n"
            "                            ('name:N:line' with --line-number, 'name:count' a file with --count), all files in\n"
            "                            one pass on the GPU (bzh_grep_many); a file that fails is named on standard error,\n"
            "                            the others are still written and the exit status is 3; not with -o, -b, -A, -B, -C, --index\n"
            "     --no-filename          with --grep and several inputs: no 'name:' in front of the lines\n"
            "     --hex                  with --search or --grep: <string> is given as hex digits\n"
            "     --count                with --search: print the number of occurrences alone; with --grep: of lines\n"
            "     -e <string>            with --search or --grep, in place of their <string> or beside it, any number of\n"
            "                            times: look for every one of the strings in one pass ('--grep -e A -e B'; a\n"
            "                            <string> that is itself '-e', '--patterns' or '--ignore-case' is given by -e)\n"
            "     --patterns <file>      as -e for every line of <file> (not hex); an empty line is an error\n"
            "     --ignore-case          with --search or --grep: 'A'..'Z' and 'a'..'z' compare equal, nothing else does\n"
            "  -E --regex                with --search or --grep: <string>, every -e and every line of --patterns are regular\n"
            "                            expressions (a subset of Python's re on bytes); a start reports its longest match of\n"
            "                            at most 256 bytes; not with --hex.  ^ $ \\A \\Z \\b \\B are Python's under re.MULTILINE:\n"
            "                            ^ and $ at the two ends of the whole decoded data and around every '\\n', \\A and \\Z\n"
            "                            at the two ends alone, \\b between a byte of [0-9A-Za-z_] and one that is none\n"
            "  -w --word-regexp          with --search or --grep: a match is neither preceded nor followed by a byte of\n"
            "                            [0-9A-Za-z_] (every length of it is tried)\n"
            "  -x --line-regexp          with --search or --grep: a match is a whole line (of an -E expression e: ^(?:e)$)\n"
            "                            Without -E the strings stay literal under -w and -x (with --hex too); -w and -x\n"
            "                            exclude each other\n"
            "                            With any of these three --search prints a third column: the number of the\n"
            "                            string, from 0 in the order given (of equal strings the first)\n"
            "     --keep      or   -k    keep the input file\n"
            "     --remove    or   -r    remove the input file\n\n"
            "     -1 to -9               block size in 100 kB units (default -9)\n"
            "     --fast                 same as -1\n"
            "     --best                 same as -9\n\n"
            "     --verbose   or   -v    accepted for compatibility\n\n"
            "  commands:\n"
            "     --help  --info  --version\n\n"
            "  notes:\n"
            "     '-' as input path reads standard in.  Without --output / --stdout the file\n"
            "     '<input_path>.bz2' is written and the input removed; with an explicit output the\n"
            "     input is kept unless --remove is given.  With --decompress the input must end in\n"
            "     '.bz2' unless --output / --stdout is given; the default output is the path without\n"
            "     that suffix, and the same keep / remove policy applies.  --recover takes the paths of\n"
            "     --decompress, writes the bytes of the intact blocks, names every lost block on standard\n"
            "     error (bit position, reason) and exits with 0 when nothing was lost, with 4 (salvage\n"
            "     written, blocks lost: the input is then kept) otherwise; it takes no level and no -d.\n"
            "     -d --stream takes the paths and the keep / remove policy of -d and bounded memory whatever\n"
            "     the sizes: a pipe is decoded as it arrives.  On a damaged input the exit status is -d's\n"
            "     and a partial output FILE is removed; on standard out the bytes decoded so far -- whole\n"
            "     blocks in front of the defect, their CRCs verified -- have been written.\n"
            "     --index while compressing holds the index in memory (40 bytes a block, 288 bytes a sync\n"
            "     point: some 2 %% of the input at the default interval) and writes the file once, at the\n"
            "     end; it runs on one GPU.  -d --index --range needs --output or --stdout and a regular\n"
            "     file as input, of which it reads only the bytes from the first block a range touches to\n"
            "     the last; the ranges' bytes are written back to back in the order given, each clipped to\n"
            "     the decoded size, and the input is kept.  An index file that is not a whole, undamaged\n"
            "     index is a filesystem error; one that does not fit the input exits as -d does for a\n"
            "     damaged input.  --search exits with 0 whether or not anything matched.  With --index (and at\n"
            "     most one --range, the bytes a match must lie wholly inside) it decodes only the blocks the\n"
            "     range touches and reads only their bytes of a regular input file; line numbers then need the\n"
            "     index to be a record index with delimiter '\\n' (banzai_amd.RecordIndex.to_bytes()), else the\n"
            "     second column is '-'.  --grep exits with 0 whether or not anything matched, as --search does;\n"
            "     a line is every byte up to and including its '\\n', a match that spans a '\\n' belongs to the line\n"
            "     of its first byte, and an unterminated last line is written as it is.  With --index (a block,\n"
            "     sync or record index of the input) the whole input goes through the indexed front and every\n"
            "     block is checked against its entry; --grep takes no --range.  GPU: $BZHIP_DEVICE (default 0), or\n"
            "     $BZHIP_DEVICES=0,1,2,... to spread the blocks over several GPUs of this node;\n"
            "     BZHIP_HUFFMAN=fixed: 2-6 Huffman tables with refinement (smaller, not banzai's exact bytes).\n\n%s\n",
            VERSION);
    exit(SUCCESS);
}
// ---------------------------------------------------------------------------------------------------------------- options
enum class Mode { ENCODE, DECODE, DECODE_STREAM, RECOVER, MAKE_INDEX, RANGE, SEARCH, GREP, MATCH, GREP_MANY };
struct Opt;
struct Options {
    std::string in_path, out_path, index_path, mkindex_path, needle;
    std::vector<std::string> more_inputs; // the inputs behind the first: --grep takes several files (judged behind the last argument)
    std::vector<std::string> pats;        // the strings of a set, in the order given (-e: hex with --hex; --patterns: as they stand)
    std::vector<bool> pat_hex;
    std::vector<const uint8_t *> pat_ptr; // the strings as the library takes them (check(): un-hexed, escaped under -w and -x)
    std::vector<size_t> pat_len;
    std::vector<bzh_range> ranges;
    bool have_in = false, in_stdin = false, have_out = false, out_stdout = false;
    int keep = -1, level = 9;
    bool level_given = false, interval_given = false, decompress = false, recover = false, dstream = false;
    uint32_t interval = 256, ctx_before = 0, ctx_after = 0;
    bool searching = false, grepping = false; // (--grep is a --search that writes lines: `searching` holds for both)
    bool use_set = false, ignore_case = false, regex = false; // regex: every string is a regular expression (bzh_regex_create_ex)
    bool word_re = false, line_re = false;                    // -w, -x: the wraps of bzh_regex_create_ex; a literal string is escaped for it
    bool needle_hex = false, count_only = false, invert = false, line_number = false, no_filename = false;
    bool only_matching = false, byte_offset = false; // -o, -b
    bool context_given = false;                      // -A, -B, -C: lines of context round every selected line
    const Opt *pending = nullptr;    // the valued option the arguments ended behind
    bzh_regex_look look{0, 0, 1, 0}; // what the automaton looks at: a --range is widened by it (check())
    Mode mode = Mode::ENCODE;        // (check())
    unsigned fold(unsigned flag) const { return ignore_case ? flag : 0; }
    unsigned regex_flags() const { return BZH_REGEX_ASSERT | (word_re ? BZH_REGEX_WORD : 0) | (line_re ? BZH_REGEX_LINE : 0); }
};
// ---------------------------------------------------------------------------------------------------------------- grammar
enum Id { FLAG, HELP, VERSION_, INFO, KEEP, REMOVE, FAST, BEST, STDOUT, END_OF_OPTIONS, OUTPUT, INDEX, MAKE_INDEX, INTERVAL, RANGE, SEARCH, GREP,
          PATTERN, PATTERNS, AFTER, BEFORE, CONTEXT };
// what a value must be.  WORD: anything; PATH: not empty, no '-' in front; PATH_OR_EMPTY: no '-' in front; NUMBER: 0 to `max`; SPAN: <number>:<number>
enum Val { NONE, WORD, PATH, PATH_OR_EMPTY, NUMBER, SPAN };
const char *const SAME = nullptr; // `at_end`: the arguments ending behind the option are refused with `needs`
const char *const NOT_ASKED = ""; // `at_end`: ... are not refused at all ('--output' as the last word is dropped)
const char *const NEEDS_INDEX_PATH = "Arguments '--index' and '--make-index' require a file path";
const char *const NEEDS_LINES = "Arguments '-A', '-B' and '-C' require a number of lines, 0 to 4294967295";
struct Opt {
    Id id;
    const char *name;      // "--name", or nullptr
    char letter;           // '-' + letter, or 0
    bool clusters;         // the letter is also read inside a cluster ('-dk'); else only standing alone
    bool as_pattern;       // standing where the <string> of --search / --grep is expected, the word is this option, not the string
    bool Options::*flag;   // FLAG: the field it sets (nullptr: none, accepted for compatibility)
    Val val;
    uint64_t max;
    const char *needs;  // the value is bad: this message
    const char *at_end; // the value is missing: SAME, NOT_ASKED or a message of its own
};
const Opt OPTS[] = {
    {HELP, "--help", 0, false, false, nullptr, NONE, 0, nullptr, SAME},
    {VERSION_, "--version", 0, false, false, nullptr, NONE, 0, nullptr, SAME},
    {INFO, "--info", 0, false, false, nullptr, NONE, 0, nullptr, SAME},
    {FLAG, "--verbose", 'v', true, false, nullptr, NONE, 0, nullptr, SAME},
    {FLAG, "--decompress", 'd', true, false, &Options::decompress, NONE, 0, nullptr, SAME},
    {FLAG, "--recover", 0, false, false, &Options::recover, NONE, 0, nullptr, SAME},
    {FLAG, "--stream", 0, false, false, &Options::dstream, NONE, 0, nullptr, SAME},
    {KEEP, "--keep", 'k', true, false, nullptr, NONE, 0, nullptr, SAME},
    {REMOVE, "--remove", 'r', true, false, nullptr, NONE, 0, nullptr, SAME},
    {FAST, "--fast", 0, false, false, nullptr, NONE, 0, nullptr, SAME}, // (-1 to -9: parse())
    {BEST, "--best", 0, false, false, nullptr, NONE, 0, nullptr, SAME},
    {STDOUT, "--stdout", 'c', true, false, nullptr, NONE, 0, nullptr, SAME},
    {END_OF_OPTIONS, "--", 0, false, false, nullptr, NONE, 0, nullptr, SAME},
    {OUTPUT, "--output", 0, false, false, nullptr, PATH_OR_EMPTY, 0, "Argument '--output' requires a file path", NOT_ASKED},
    {INDEX, "--index", 0, false, false, nullptr, PATH, 0, "Argument '--index' requires a file path", NEEDS_INDEX_PATH},
    {MAKE_INDEX, "--make-index", 0, false, false, nullptr, PATH, 0, "Argument '--make-index' requires a file path", NEEDS_INDEX_PATH},
    {INTERVAL, "--interval", 0, false, false, nullptr, NUMBER, 32767, "Argument '--interval' requires a number of groups, 0 to 32767", SAME},
    {RANGE, "--range", 0, false, false, nullptr, SPAN, 0, "Argument '--range' requires <offset>:<length>, both in bytes", SAME},
    {SEARCH, "--search", 0, false, false, nullptr, WORD, 0, "Argument '--search' requires a string", SAME},
    {GREP, "--grep", 0, false, false, nullptr, WORD, 0, "Argument '--grep' requires a string", SAME},
    {FLAG, "--invert", 0, false, false, &Options::invert, NONE, 0, nullptr, SAME},
    {FLAG, "--line-number", 0, false, false, &Options::line_number, NONE, 0, nullptr, SAME},
    {FLAG, "--only-matching", 'o', false, false, &Options::only_matching, NONE, 0, nullptr, SAME},
    {FLAG, "--byte-offset", 'b', false, false, &Options::byte_offset, NONE, 0, nullptr, SAME},
    {FLAG, "--hex", 0, false, false, &Options::needle_hex, NONE, 0, nullptr, SAME},
    {FLAG, "--count", 0, false, false, &Options::count_only, NONE, 0, nullptr, SAME},
    {FLAG, "--no-filename", 0, false, false, &Options::no_filename, NONE, 0, nullptr, SAME},
    {PATTERN, nullptr, 'e', false, true, nullptr, WORD, 0, "Argument '-e' requires a string", SAME},
    {PATTERNS, "--patterns", 0, false, true, nullptr, WORD, 0, "Argument '--patterns' requires a file path", SAME},
    {FLAG, "--ignore-case", 0, false, true, &Options::ignore_case, NONE, 0, nullptr, SAME},
    {FLAG, "--regex", 'E', false, true, &Options::regex, NONE, 0, nullptr, SAME},
    {FLAG, "--word-regexp", 'w', false, true, &Options::word_re, NONE, 0, nullptr, SAME},
    {FLAG, "--line-regexp", 'x', false, true, &Options::line_re, NONE, 0, nullptr, SAME},
    {AFTER, "--after-context", 'A', false, false, nullptr, NUMBER, UINT32_MAX, NEEDS_LINES, SAME},
    {BEFORE, "--before-context", 'B', false, false, nullptr, NUMBER, UINT32_MAX, NEEDS_LINES, SAME},
    {CONTEXT, "--context", 'C', false, false, nullptr, NUMBER, UINT32_MAX, NEEDS_LINES, SAME},
};

// the row of a word that is an option as a whole ("--name", or '-' and one letter), or of a letter inside a cluster
const Opt *find(const std::string &a, bool in_cluster = false)
{
    const bool letter = in_cluster || (a.size() == 2 && a[0] == '-' && a[1] != '-');
    for (const Opt &r : OPTS)
        if (letter ? r.letter == a.back() && (r.clusters || !in_cluster) : r.name && a == r.name) return &r;
    return nullptr;
}

// a decimal number of at most 20 digits that fits 64 bits, nothing else
bool number(const std::string &t, uint64_t *v)
{
    if (t.empty() || t.size() > 20) return false;
    uint64_t x = 0;
    for (char ch : t) {
        if (ch < '0' || ch > '9') return false;
        const uint64_t d = (uint64_t)(ch - '0');
        if (x > (UINT64_MAX - d) / 10) return false;
        x = x * 10 + d;
    }
    *v = x;
    return true;
}
void set_input(Options &o, const std::string &p, bool is_stdin)
{
    if (o.have_in) {
        if (is_stdin || o.in_stdin) die(ERR_ARGS, "Only one input may be specified");
        o.more_inputs.push_back(p);
        return;
    }
    o.have_in = true;
    o.in_stdin = is_stdin;
    o.in_path = p;
}
void set_output(Options &o, const std::string &p, bool is_stdout)
{
    if (o.have_out && !(o.out_stdout && is_stdout)) die(ERR_ARGS, "Only one output may be specified");
    o.have_out = true;
    o.out_stdout = is_stdout;
    o.out_path = p;
}
void add_pattern(Options &o, const std::string &s, bool hex) { o.pats.push_back(s), o.pat_hex.push_back(hex); }

// --patterns: every line of the file a string
void read_patterns(Options &o, const std::string &path)
{
    std::vector<uint8_t> bytes;
    FILE *pf = open_file(path);
    read_all(pf, bytes); // (what was read up to a failure is taken)
    fclose(pf);
    const std::string all(bytes.begin(), bytes.end());
    size_t line = 1;
    for (size_t at = 0; at < all.size(); line++) {
        size_t end = all.find('\n', at);
        if (end == std::string::npos) end = all.size();
        if (end == at) die(ERR_ARGS, "'--patterns': line " + std::to_string(line) + " of " + path + " is empty");
        add_pattern(o, all.substr(at, end - at), false);
        at = end + 1;
    }
}

// an option without a value: what it sets.  One with a value waits for the next word (take_value)
void apply(Options &o, const Opt &r)
{
    if (r.val != NONE) o.pending = &r;
    else if (r.flag) o.*r.flag = true;
    else if (r.id == HELP) usage(true);
    else if (r.id == VERSION_) die(SUCCESS, VERSION);
    else if (r.id == INFO)
        die(SUCCESS, std::string(TAGLINE) +
                         "\n\nBlocks are suffix-sorted by prefix doubling with radix sorts, move-to-front\n"
                         "coded and Huffman coded by HIP kernels (libbzhip.so); the stream is bit-identical\n"
                         "to banzai 0.3.1's.\n\n" + VERSION);
    else if (r.id == KEEP || r.id == REMOVE) o.keep = r.id == KEEP;
    else if (r.id == FAST || r.id == BEST) o.level = r.id == FAST ? 1 : 9, o.level_given = true;
    else if (r.id == STDOUT) set_output(o, "", true);
}

// the word behind a valued option: held to the row's Val, then what it sets
void take_value(Options &o, const Opt &r, const std::string &a)
{
    uint64_t v = 0;
    bzh_range span{0, 0};
    const size_t colon = a.find(':');
    const bool dash = !a.empty() && a[0] == '-';
    const bool bad = r.val == PATH            ? a.empty() || dash
                     : r.val == PATH_OR_EMPTY ? dash
                     : r.val == NUMBER        ? !number(a, &v) || v > r.max
                     : r.val == SPAN          ? colon == std::string::npos || !number(a.substr(0, colon), &span.off) || !number(a.substr(colon + 1), &span.len)
                                              : false;
    if (bad) die(ERR_ARGS, r.needs);
    if (r.id == OUTPUT) set_output(o, a, false);
    else if (r.id == INDEX || r.id == MAKE_INDEX) {
        std::string &dst = r.id == INDEX ? o.index_path : o.mkindex_path;
        if (!dst.empty()) die(ERR_ARGS, std::string("'") + r.name + "' may be given once");
        dst = a;
    } else if (r.id == INTERVAL) o.interval = (uint32_t)v, o.interval_given = true;
    else if (r.id == AFTER || r.id == BEFORE || r.id == CONTEXT) {
        if (r.id != BEFORE) o.ctx_after = (uint32_t)v;
        if (r.id != AFTER) o.ctx_before = (uint32_t)v;
        o.context_given = true;
    } else if (r.id == RANGE) o.ranges.push_back(span);
    else if (r.id == PATTERN) add_pattern(o, a, true), o.use_set = true;
    else if (r.id == PATTERNS) read_patterns(o, a), o.use_set = true;
    else if (r.id == SEARCH || r.id == GREP) {
        const bool grep = r.id == GREP;
        if (o.searching) die(ERR_ARGS, o.grepping != grep ? "'--grep' and '--search' exclude each other" : "'--search' and '--grep' may be given once");
        o.searching = true;
        o.grepping = grep;
        const Opt *w = find(a); // (no <string> of its own: the word is an option of the set, whose strings follow)
        if (w && w->as_pattern) apply(o, *w);
        else o.needle = a, add_pattern(o, a, true);
    }
}

Options parse(int argc, char **argv)
{
    Options o;
    bool options_ended = false; // behind '--' every word is an input
    for (int k = 1; k < argc; k++) {
        const std::string a = argv[k];
        const bool option = !options_ended && a.size() > 1 && a[0] == '-';
        const Opt *r = option ? find(a) : nullptr;
        if (o.pending) {
            r = o.pending;
            o.pending = nullptr; // (the word may itself be a valued option: '--search -e')
            take_value(o, *r, a);
        } else if (r) {
            if (r->id == END_OF_OPTIONS) options_ended = true;
            else apply(o, *r);
        } else if (option && a[1] == '-') {
            die(ERR_ARGS, "Unrecognised argument " + a);
        } else if (option) { // a cluster: the letters that cluster, and -1 to -9
            for (size_t c = 1; c < a.size(); c++) {
                if ((r = find(std::string(1, a[c]), true))) apply(o, *r);
                else if (a[c] >= '1' && a[c] <= '9') o.level = a[c] - '0', o.level_given = true;
                else die(ERR_ARGS, std::string("Flag '") + a[c] + "' is not valid");
            }
        } else {
            set_input(o, a == "-" && !options_ended ? "" : a, a == "-" && !options_ended);
        }
    }
    return o;
}
// ---------------------------------------------------------------------------------------------------------------- checks
const char *const GREP_TAKES = "'--grep' takes an input, '--hex', '--invert', '--count', '--line-number', '-o', '-b', '-A', '-B', '-C' and '--index', nothing else";
void unhex(std::string &s)
{
    std::string raw;
    auto nib = [](char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; };
    if (s.size() % 2) die(ERR_ARGS, "Argument '--search' with '--hex' requires an even number of hex digits");
    for (size_t c = 0; c < s.size(); c += 2) {
        if (nib(s[c]) < 0 || nib(s[c + 1]) < 0) die(ERR_ARGS, "Argument '--search' with '--hex' requires hex digits");
        raw.push_back((char)(nib(s[c]) * 16 + nib(s[c + 1])));
    }
    s = raw;
}

// --search / --grep: what goes with them; then the strings un-hexed, escaped under -w / -x, and compiled once on the host when they are
// expressions: what that refuses is refused before a file is read, and a --range knows its neighbours
void check_search(Options &o)
{
    if (o.decompress || o.recover || o.dstream || o.have_out || !o.mkindex_path.empty() || o.level_given || o.interval_given || o.keep == 0)
        die(ERR_ARGS, o.grepping ? GREP_TAKES : "'--search' takes an input, '--hex', '--count', '--index' and one '--range', nothing else");
    if (o.ranges.size() > 1 || (!o.ranges.empty() && o.index_path.empty())) die(ERR_ARGS, "'--search' takes one '--range', with the '--index' of the input");
    if (!o.index_path.empty() && o.in_stdin) die(ERR_ARGS, "'--search --index' reads parts of a file: standard in cannot be the input");
    if (o.needle_hex && !o.use_set) unhex(o.needle);
    if (!o.use_set && (o.needle.empty() || o.needle.size() > BZH_SEARCH_MAX_PATTERN)) die(ERR_ARGS, "Argument '--search' requires a string of 1 to 256 bytes");
    for (size_t k = 0; o.use_set && k < o.pats.size(); k++) {
        if (o.needle_hex && o.pat_hex[k]) unhex(o.pats[k]);
        if (o.pats[k].empty() || o.pats[k].size() > (o.regex ? BZH_REGEX_MAX_EXPR : BZH_SEARCH_MAX_PATTERN))
            die(ERR_ARGS, "string " + std::to_string(k) + (o.regex ? " does not hold 1 to 4096 bytes" : " does not hold 1 to 256 bytes"));
    }
    if (o.use_set && o.pats.size() > BZH_PATSET_MAX_PATTERNS) die(ERR_ARGS, "more than 65536 strings");
    if ((o.word_re || o.line_re) && !o.regex) { // a literal string under a wrap goes the regex way, every byte as \xHH: 256 bytes become 1,024
        for (std::string &q : o.pats) {
            std::string esc;
            char h[8];
            for (unsigned char ch : q) snprintf(h, sizeof h, "\\x%02X", ch), esc += h;
            q = esc;
        }
        o.regex = true;
    }
    for (const std::string &q : o.pats) o.pat_ptr.push_back((const uint8_t *)q.data()), o.pat_len.push_back(q.size());
    char why[256] = "";
    const int rc = !o.regex ? BZH_OK
                            : bzh_regex_check_ex(o.pat_ptr.data(), o.pat_len.data(), o.pats.size(), o.fold(BZH_REGEX_FOLD_ASCII), 0, o.regex_flags(), nullptr, &o.look, why, sizeof why);
    if (rc != BZH_OK) die(rc == BZH_E_ARG ? ERR_ARGS : ERR_OUTPUT, std::string("error during search: ") + bzh_strerror(rc) + ": " + why);
}

// the checks behind the last argument.  Their order is behaviour: of two errors in one argv the first one here is reported
void check(Options &o)
{
    const bool several = !o.more_inputs.empty();
    if (several && !o.grepping) die(ERR_ARGS, "Only one input may be specified");
    if (o.no_filename && !o.grepping) die(ERR_ARGS, "'--no-filename' goes with '--grep'");
    // several inputs go through one bzh_grep_many: what it does not do is refused by name
    const char *one = o.only_matching ? "-o" : o.byte_offset ? "-b" : o.context_given ? "-A', '-B' and '-C" : !o.index_path.empty() ? "--index" : nullptr;
    if (several && one) die(ERR_ARGS, std::string("'") + one + "' takes one input: several inputs go with '--grep' and '--hex', '--invert', '--count', '--line-number', '--no-filename'");
    if (o.pending && o.pending->at_end != NOT_ASKED) die(ERR_ARGS, o.pending->at_end == SAME ? o.pending->needs : o.pending->at_end);
    if (o.word_re && o.line_re) die(ERR_ARGS, "'-w' and '-x' exclude each other");
    if ((o.word_re || o.line_re) && !o.searching) die(ERR_ARGS, "'-w' and '-x' go with '--search' or '--grep'");
    o.use_set = o.use_set || o.ignore_case || o.regex || o.word_re || o.line_re;
    if (o.use_set && !o.searching) die(ERR_ARGS, "'-e', '-E', '--patterns' and '--ignore-case' go with '--search' or '--grep'");
    if (o.regex && o.needle_hex) die(ERR_ARGS, "'-E' and '--hex' exclude each other: a regular expression writes a byte as \\xHH");
    if (o.use_set && o.pats.empty()) die(ERR_ARGS, "'--search' and '--grep' require a string, a '-e' or a '--patterns'");
    if (!o.have_in) die(ERR_ARGS, "An input must be specified");
    if ((o.needle_hex || o.count_only) && !o.searching) die(ERR_ARGS, "'--hex' and '--count' go with '--search' or '--grep'");
    if ((o.invert || o.line_number) && !o.grepping) die(ERR_ARGS, "'--invert' and '--line-number' go with '--grep'");
    if (o.context_given && !o.grepping) die(ERR_ARGS, "'-A', '-B' and '-C' go with '--grep'");
    if ((o.only_matching || o.byte_offset) && !o.grepping) die(ERR_ARGS, "'-o' and '-b' go with '--grep'");
    if (o.only_matching && (o.invert || o.context_given)) die(ERR_ARGS, "'-o' writes the matched parts alone: it does not go with '--invert', '-A', '-B' or '-C'");
    if (o.grepping && !o.ranges.empty()) die(ERR_ARGS, GREP_TAKES);
    if (o.searching) check_search(o);
    const bool by_range = !o.ranges.empty() && !o.searching, make_index = !o.mkindex_path.empty(), indexed = !o.index_path.empty();
    if (by_range && !indexed) die(ERR_ARGS, "'--range' needs the '--index' of the input");
    if (by_range && (o.dstream || o.recover)) die(ERR_ARGS, "'--range' goes with neither '--stream' nor '--recover'");
    if (by_range && !o.decompress) die(ERR_ARGS, "'--range' goes with '--decompress'");
    if (by_range && o.in_stdin) die(ERR_ARGS, "'--range' reads parts of a file: standard in cannot be the input");
    if (by_range && !o.have_out) die(ERR_ARGS, "'--range' needs '--output' or '--stdout'");
    if (indexed && !by_range && !o.searching && (o.decompress || o.recover)) die(ERR_ARGS, "With '--decompress' an '--index' is read by '--range'; '--recover' takes none");
    if (make_index && (o.decompress || o.recover || o.dstream || o.have_out || indexed || o.level_given))
        die(ERR_ARGS, "'--make-index' takes an input, a path and '--interval', nothing else");
    if (o.interval_given && !make_index && (!indexed || o.decompress)) die(ERR_ARGS, "'--interval' goes with '--make-index', or with '--index' while compressing");
    if (o.recover && o.decompress) die(ERR_ARGS, "'--recover' and '--decompress' exclude each other");
    if (o.dstream && o.recover) die(ERR_ARGS, "'--stream' and '--recover' exclude each other");
    if (o.dstream && !o.decompress) die(ERR_ARGS, "'--stream' goes with '--decompress'");
    if (o.recover && o.level_given) die(ERR_ARGS, "'--recover' takes no block size: a block is held to what the format allows");
    o.mode = several ? Mode::GREP_MANY : o.grepping && o.only_matching && !o.count_only ? Mode::MATCH : o.grepping ? Mode::GREP : o.searching ? Mode::SEARCH
             : by_range ? Mode::RANGE : make_index ? Mode::MAKE_INDEX : o.dstream ? Mode::DECODE_STREAM : o.recover ? Mode::RECOVER
             : o.decompress ? Mode::DECODE : Mode::ENCODE;
}
// ---------------------------------------------------------------------------------------------------------------- device
// The context and the optional pattern set of a run.  die() ends in exit(), which runs no destructor: every way out closes by hand.
struct Device {
    bzh_ctx *ctx = nullptr;
    bzh_patset *set = nullptr;
    const char *doing; // "error during ...: ", in front of every message
    Device(const char *doing_, int level = 9) : doing(doing_)
    {
        const char *dv = getenv("BZHIP_DEVICE");
        const int rc = bzh_create(&ctx, dv ? atoi(dv) : 0, level, 0);
        if (rc != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(rc));
    }
    void close() { bzh_patset_destroy(set), bzh_destroy(ctx), set = nullptr, ctx = nullptr; }
    // the message is worded first (closing the context frees its text), then the set and the context go, then the process
    [[noreturn]] void fail(const std::string &what, int code = ERR_OUTPUT)
    {
        const std::string msg = std::string(doing) + what;
        close();
        die(code, msg);
    }
    [[noreturn]] void fail(int rc, int code = ERR_OUTPUT) { fail(std::string(bzh_strerror(rc)) + ": " + bzh_last_error(ctx), code); }
    void expect(int rc) { if (rc != BZH_OK) fail(rc); }
};

// Guess the rooms, call, and on BZH_E_CAP grow them to what the call reported and call again: `attempts` calls at the most
template <class Call, class Grow> int with_retry(int attempts, Call call, Grow grow)
{
    for (int attempt = 1;; attempt++) {
        const int rc = call();
        if (rc != BZH_E_CAP || attempt >= attempts) return rc;
        grow();
    }
}
// ---------------------------------------------------------------------------------------------------------------- files
FILE *open_input(const Options &o) { return o.in_stdin ? stdin : open_file(o.in_path); }
// the whole input, file or standard in, closed behind the read; `doing` words a failed read
std::vector<uint8_t> read_input(const Options &o, FILE *inf, const char *doing)
{
    std::vector<uint8_t> data;
    if (!read_all(inf, data)) die(ERR_OUTPUT, std::string(doing) + "read failed");
    if (!o.in_stdin) fclose(inf);
    return data;
}

// the size of the input, which must be a regular file: `who` ('--range', '--search --index') reads parts of it
uint64_t regular_size(const std::string &path, const char *who)
{
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + path + ": " + strerror(errno));
    if (!S_ISREG(sb.st_mode)) die(ERR_ARGS, std::string("'") + who + "' reads parts of a regular file: " + path + " is none");
    return (uint64_t)sb.st_size;
}

// the bytes [lo, hi) of a regular file of `size` bytes, as an index names them (checked before anything is sized by them), or all of it
std::vector<uint8_t> read_span(const std::string &path, uint64_t size, uint64_t lo, uint64_t hi, const char *doing, bool whole = false)
{
    if (hi < lo || hi > size) die(ERR_OUTPUT, std::string(doing) + "the index names bytes behind the end of " + path + ": it is not this file's");
    FILE *rf = open_file(path);
    if (whole) lo = 0, hi = size;
    std::vector<uint8_t> data;
    try { data.resize((size_t)(hi - lo)); } catch (const std::bad_alloc &) { die(ERR_OUTPUT, std::string(doing) + "out of memory"); }
    if (!data.empty() && (fseeko(rf, (off_t)lo, SEEK_SET) != 0 || fread(data.data(), 1, data.size(), rf) != data.size()))
        die(ERR_OUTPUT, std::string(doing) + "read failed");
    fclose(rf);
    return data;
}

// where the output goes: the file of --output, the name derived from the input's, or standard out
struct Output { bool to_file; std::string path; };
Output output_of(const Options &o, const std::string &derived) { return o.have_out ? Output{!o.out_stdout, o.out_path} : Output{!o.in_stdin, derived}; }
FILE *open_output(const Output &out, Device *dev = nullptr) // (a device that is open is closed before the exit)
{
    FILE *f = out.to_file ? fopen(out.path.c_str(), "wb") : stdout;
    if (f) return f;
    const std::string msg = "[filesystem error] cannot create " + out.path + ": " + strerror(errno);
    if (dev) dev->close();
    die(ERR_FILESYSTEM, msg);
}
// bytes -> the output, flushed and closed; `doing` words a failed write
void write_output(FILE *f, const uint8_t *p, size_t n, const char *doing)
{
    if ((n && fwrite(p, 1, n, f) != n) || fflush(f) != 0) die(ERR_OUTPUT, std::string(doing) + "write failed");
    if (f != stdout) fclose(f);
}

// the input is kept with an explicit output and removed without one, unless --keep or --remove says otherwise
void finish_input(const Options &o)
{
    const bool keep_input = o.keep >= 0 ? o.keep == 1 : o.have_out; // bnz/src/main.rs:292-300
    if (!keep_input && !o.in_stdin && remove(o.in_path.c_str()) != 0) die(ERR_OUTPUT, "error deleting input file: " + std::string(strerror(errno)));
}

// entries, points, interval, consumed -> an index file, or the filesystem error
void write_index(const std::string &path, const std::vector<bzh_index_entry> &ent, const std::vector<bzh_sync_point> &pts, uint32_t iv, uint64_t consumed)
{
    const size_t need = bzh_index_blob_size(ent.size(), pts.size(), iv);
    std::unique_ptr<uint8_t[]> blob(need ? new (std::nothrow) uint8_t[need] : nullptr);
    size_t got = 0;
    if (!blob || bzh_index_blob_write(ent.data(), ent.size(), pts.data(), pts.size(), iv, consumed, blob.get(), need, &got) != BZH_OK)
        die(ERR_FILESYSTEM, "[filesystem error] the index does not fit in memory");
    FILE *xf = fopen(path.c_str(), "wb");
    if (!xf) die(ERR_FILESYSTEM, "[filesystem error] cannot create " + path + ": " + strerror(errno));
    const bool ok = fwrite(blob.get(), 1, got, xf) == got;
    if (fclose(xf) != 0 || !ok) {
        remove(path.c_str());
        die(ERR_FILESYSTEM, "[filesystem error] write to " + path + " failed");
    }
}
struct Index {
    std::vector<bzh_index_entry> entries;
    std::vector<bzh_sync_point> points;
    std::vector<uint64_t> rec_cum; // a record index: the records in front of every entry, and behind the last
    bool is_record_index = false;
    uint32_t delim = 0, interval = 0;
    uint64_t consumed = 0;
};
enum Records { NO_RECORDS, ANY_RECORDS, LINE_RECORDS }; // what load_index admits of a record index: none, any, or of delimiter '\n' alone

// an index file -> Index.  A block or sync index is bzh_index_blob_*'s; a record index is an envelope round one:
// "BZhREC\r\n" | u32 version 1 | u32 delim | u64 entries | u64 records | u32 CRC-32 | u32 0 | an index blob | the table of entries + 1 words
Index load_index(const std::string &path, Records accept)
{
    std::vector<uint8_t> blob;
    FILE *xf = open_file(path);
    const bool xok = read_all(xf, blob);
    fclose(xf);
    if (!xok) die(ERR_FILESYSTEM, "[filesystem error] cannot read " + path);
    const std::string damaged = "[filesystem error] " + path + " is not a whole, undamaged index file";
    Index ix;
    const uint8_t *ib = blob.data();
    size_t in = blob.size();
    auto get = [&blob](size_t at, int bytes) {
        uint64_t v = 0;
        for (int j = bytes - 1; j >= 0; j--) v = v << 8 | blob[at + j];
        return v;
    };
    ix.is_record_index = accept != NO_RECORDS && blob.size() >= 40 && memcmp(blob.data(), "BZhREC\r\n", 8) == 0;
    if (ix.is_record_index) {
        const uint64_t nent = get(16, 8);
        if (get(8, 4) != 1 || get(36, 4) != 0 || nent >= blob.size() / 8 || blob.size() < 40 + 8 * (nent + 1)) die(ERR_FILESYSTEM, damaged);
        uint32_t crc = 0xFFFFFFFFu; // zlib's CRC-32 over the header with its CRC field zero and everything behind it
        for (size_t at = 0; at < blob.size(); at++) {
            crc ^= at >= 32 && at < 36 ? 0u : blob[at];
            for (int j = 0; j < 8; j++) crc = crc >> 1 ^ (0xEDB88320u & (0u - (crc & 1u)));
        }
        if ((crc ^ 0xFFFFFFFFu) != (uint32_t)get(32, 4)) die(ERR_FILESYSTEM, damaged);
        ix.delim = (uint32_t)get(12, 4);
        if (ix.delim != '\n' && accept == LINE_RECORDS) die(ERR_ARGS, "'--search' counts lines: " + path + " holds records of another delimiter");
        ix.rec_cum.resize((size_t)nent + 1);
        for (size_t e = 0; e <= nent; e++) ix.rec_cum[e] = get(blob.size() - 8 * (nent + 1) + 8 * e, 8);
        ib = blob.data() + 40;
        in = blob.size() - 40 - 8 * ((size_t)nent + 1);
    }
    size_t count = 0, npts = 0; // the counts first, then the entries and the points into rooms of exactly that size
    int rs = bzh_index_blob_read(in ? ib : &NOTHING, in, nullptr, 0, &count, nullptr, 0, &npts, &ix.interval, &ix.consumed);
    ix.entries.resize(count), ix.points.resize(npts);
    if (rs == BZH_E_CAP) rs = bzh_index_blob_read(ib, in, ix.entries.data(), count, &count, ix.points.data(), npts, &npts, &ix.interval, &ix.consumed);
    if (rs != BZH_OK || (ix.is_record_index && ix.rec_cum.size() != count + 1)) die(ERR_FILESYSTEM, damaged);
    return ix;
}
// ---------------------------------------------------------------------------------------------------------------- encode
// $BZHIP_DEVICES = "0,1,2,3": the GPUs of this node the blocks are spread over (bzh_create_multi: one host thread and context per device
// inside the library; the stream is the one a single device writes).  That path holds the whole input in memory
int run_encode_multi(const Options &o, FILE *inf, FILE *outf, const std::vector<int> &devices)
{
    const char *doing = "error during compression: ";
    std::vector<uint8_t> data;
    if (!read_all(inf, data)) die(ERR_OUTPUT, std::string(doing) + "read failed");
    bzh_multi *m = nullptr;
    int ms = bzh_create_multi(&m, devices.data(), (int)devices.size(), o.level);
    if (ms != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(ms));
    const size_t n = data.size(), cap = n + n / 4 + (n / 70000 + 4) * 4096 + 65536;
    std::unique_ptr<uint8_t[]> out(new (std::nothrow) uint8_t[cap]);
    size_t got = 0;
    ms = out ? bzh_multi_encode(m, n ? data.data() : &NOTHING, n, out.get(), cap, &got, nullptr) : BZH_E_NOMEM;
    const std::string msg = ms == BZH_OK ? "" : std::string(doing) + bzh_strerror(ms) + ": " + bzh_multi_last_error(m);
    bzh_destroy_multi(m);
    if (ms != BZH_OK) die(ERR_OUTPUT, msg);
    if (got && fwrite(out.get(), 1, got, outf) != got) die(ERR_OUTPUT, std::string(doing) + "write failed");
    if (!o.in_stdin) fclose(inf);
    write_output(outf, nullptr, 0, doing);
    finish_input(o);
    return SUCCESS;
}

// The input is fed to bzh_stream_feed in reads of CHUNK (like the reference's BufRead loop, memory stays bounded, pipes and inputs
// larger than memory work, and reading overlaps with the GPU passes); the stream bytes are written as they become final
int run_encode(const Options &o)
{
    const char *doing = "error during compression: ";
    FILE *inf = open_input(o);
    FILE *outf = open_output(output_of(o, o.in_path + ".bz2"));
    // not flags: the reference's grammar stays.  BZHIP_HUFFMAN=fixed: the opt-in Huffman mode (2..6 tables, real refinement: smaller files, no longer banzai's bits)
    const char *hm = getenv("BZHIP_HUFFMAN"), *dl = getenv("BZHIP_DEVICES");
    const bool fixed = hm && std::string(hm) == "fixed", with_index = !o.index_path.empty();
    std::vector<int> devices;
    for (const char *q = dl ? dl : ""; *q;) {
        char *e = nullptr;
        const long v = strtol(q, &e, 10);
        if (e == q) break;
        devices.push_back((int)v);
        q = *e == ',' ? e + 1 : e;
        if (*e && *e != ',') break;
    }
    if (devices.size() > 1 && !fixed && !with_index) return run_encode_multi(o, inf, outf, devices);
    Device dev(doing, o.level);
    int st = fixed ? bzh_set_mode(dev.ctx, BZH_MODE_FIXED) : BZH_OK;
    if (st == BZH_OK) st = with_index ? bzh_stream_begin_index(dev.ctx, o.interval) : bzh_stream_begin(dev.ctx);
    if (st != BZH_OK) dev.fail(bzh_strerror(st));
    // --index: what every feed made final is taken at once; the whole index waits here and is written once, at the end (its header holds a CRC over it all)
    std::vector<bzh_index_entry> ix_ent;
    std::vector<bzh_sync_point> ix_pts;
    uint64_t written = 0;
    // plain arrays, not vectors: value-initialising the worst-case output bound (and copying it when it grows) cost more than encoding a 100 MB file
    std::unique_ptr<uint8_t[]> in(new uint8_t[CHUNK]), out;
    size_t out_cap = 0;
    for (bool eof = false; !eof;) {
        const size_t k = fread(in.get(), 1, CHUNK, inf);
        if (k < CHUNK) {
            if (ferror(inf)) dev.fail("read failed");
            eof = true;
        }
        const size_t cap = bzh_stream_bound(dev.ctx, k); // depends on what is pending and in flight: ask every time
        if (out_cap < cap) {
            out.reset(); // (nothing in it is still needed)
            out_cap = cap + cap / 2;
            out.reset(new (std::nothrow) uint8_t[out_cap]);
            if (!out) dev.fail("out of memory");
        }
        size_t got = 0, ne = 0, np = 0;
        dev.expect(bzh_stream_feed(dev.ctx, in.get(), k, eof ? 1 : 0, out.get(), out_cap, &got));
        if (got && fwrite(out.get(), 1, got, outf) != got) dev.fail("write failed");
        written += got;
        if (!with_index) continue;
        st = bzh_stream_index_pending(dev.ctx, &ne, &np);
        if (st != BZH_OK) dev.fail(bzh_strerror(st));
        const size_t e0 = ix_ent.size(), p0 = ix_pts.size();
        ix_ent.resize(e0 + ne);
        ix_pts.resize(p0 + np);
        dev.expect(bzh_stream_index_take(dev.ctx, ix_ent.data() + e0, ne, &ne, ix_pts.data() + p0, np, &np));
    }
    dev.close();
    if (with_index) write_index(o.index_path, ix_ent, ix_pts, o.interval, written);
    if (!o.in_stdin) fclose(inf);
    write_output(outf, nullptr, 0, doing);
    finish_input(o);
    return SUCCESS;
}
// ---------------------------------------------------------------------------------------------------------------- decode
// -d, -d --stream and --recover write to --output, to standard out, or to the input's path without its '.bz2'
Output decoded_output(const Options &o)
{
    if (o.have_out || o.in_stdin) return output_of(o, "");
    if (o.in_path.size() < 5 || o.in_path.compare(o.in_path.size() - 4, 4, ".bz2") != 0)
        die(ERR_ARGS, std::string("With ") + (o.recover ? "--recover" : "--decompress") + " the input path must end in '.bz2' unless --output or --stdout is given");
    return output_of(o, o.in_path.substr(0, o.in_path.size() - 4));
}

// -d: the whole input in memory, one bzh_decode into 6 n + 65,536 bytes, a second one if that guess was short
int run_decode(const Options &o)
{
    const char *doing = "error during decompression: ";
    FILE *inf = open_input(o);
    const Output dest = decoded_output(o);
    const std::vector<uint8_t> data = read_input(o, inf, doing);
    Device dev(doing);
    const size_t n = data.size();
    size_t cap = 6 * n + 65536, got = 0;
    std::unique_ptr<uint8_t[]> out;
    auto call = [&] {
        out.reset(new (std::nothrow) uint8_t[cap ? cap : 1]);
        return out ? bzh_decode(dev.ctx, n ? data.data() : &NOTHING, n, out.get(), cap, &got, nullptr) : BZH_E_NOMEM;
    };
    dev.expect(with_retry(2, call, [&] { cap = got; })); // (a failure leaves the input where it is, and no output is created)
    dev.close();
    write_output(open_output(dest), out.get(), got, doing);
    finish_input(o);
    return SUCCESS;
}

// --recover: one bzh_recover with a guessed room for the bytes and for the report; BZH_E_CAP names what either needs
int run_recover(const Options &o)
{
    const char *doing = "error during recovery: ";
    FILE *inf = open_input(o);
    const Output dest = decoded_output(o);
    const std::vector<uint8_t> data = read_input(o, inf, doing);
    Device dev(doing);
    const size_t n = data.size();
    size_t cap = 6 * n + 65536, got = 0, count = 0, kept = 0, lost = 0;
    std::unique_ptr<uint8_t[]> out;
    std::vector<bzh_recover_entry> ent(n / 1000 + 64);
    auto call = [&] {
        out.reset(new (std::nothrow) uint8_t[cap ? cap : 1]);
        return out ? bzh_recover(dev.ctx, n ? data.data() : &NOTHING, n, out.get(), cap, &got, ent.data(), ent.size(), &count) : BZH_E_NOMEM;
    };
    auto grow = [&] { cap = std::max(cap, got), ent.resize(std::max(ent.size(), count)); };
    dev.expect(with_retry(3, call, grow));
    bzh_recover_stats rs{};
    dev.expect(bzh_get_recover_stats(dev.ctx, &rs));
    for (size_t k = 0; k < count; k++) {
        const bzh_recover_entry &e = ent[k];
        kept += e.kind == 0;
        if (e.kind == 0) continue;
        lost++;
        const char *why = e.kind == BZH_LOST_TRUNC ? "truncated" : e.kind == BZH_LOST_FORMAT ? "field outside the format"
                        : e.kind == BZH_LOST_BLOCK_CRC ? "block CRC mismatch" : e.kind == BZH_LOST_RANDOMISED ? "randomised block" : "error";
        fprintf(stderr, "lost: block at bit %llu: %s (found at bit %llu)\n", (unsigned long long)e.bit_pos, why, (unsigned long long)e.err_bit);
    }
    fprintf(stderr, "recovered: %zu blocks kept, %zu lost, %zu bytes, %llu streams whole\n", kept, lost, got, (unsigned long long)rs.streams_ok);
    dev.close();
    write_output(open_output(dest), out.get(), got, doing);
    if (lost) return LOST_BLOCKS; // (a damaged archive of which blocks were lost is never removed)
    finish_input(o);
    return SUCCESS;
}

// -d --stream: bzh_dstream_feed through two fixed buffers, 8 MiB reads and 16 MiB writes; bounded memory whatever the sizes
int run_decode_stream(const Options &o)
{
    const char *doing = "error during decompression: ";
    FILE *inf = open_input(o);
    const Output dest = decoded_output(o);
    Device dev(doing);
    FILE *sf = stdout;
    auto fail = [&](const std::string &what) { // no partial output file is left behind
        if (sf != stdout) fclose(sf), remove(dest.path.c_str());
        dev.fail(what);
    };
    auto expect = [&](int rc) { if (rc != BZH_OK) fail(std::string(bzh_strerror(rc)) + ": " + bzh_last_error(dev.ctx)); };
    expect(bzh_dstream_begin(dev.ctx));
    sf = open_output(dest, &dev);
    const size_t IN_CHUNK = (size_t)8 << 20, OUT_CHUNK = (size_t)16 << 20;
    std::unique_ptr<uint8_t[]> ibuf(new uint8_t[IN_CHUNK]), obuf(new uint8_t[OUT_CHUNK]);
    int done = 0;
    for (bool eof = false; !done;) {
        size_t k = 0;
        if (!eof) {
            k = fread(ibuf.get(), 1, IN_CHUNK, inf);
            if (k < IN_CHUNK && ferror(inf)) fail("read failed");
            eof = k < IN_CHUNK;
        }
        for (size_t off = 0;;) { // until the chunk is used and nothing more comes out
            size_t used = 0, got = 0;
            expect(bzh_dstream_feed(dev.ctx, ibuf.get() + off, k - off, eof ? 1 : 0, &used, obuf.get(), OUT_CHUNK, &got, &done));
            if (got && fwrite(obuf.get(), 1, got, sf) != got) fail("write failed");
            off += used;
            if (done || (off == k && got < OUT_CHUNK && !eof)) break;
        }
    }
    if (fflush(sf) != 0) fail("write failed");
    dev.close();
    if (!o.in_stdin) fclose(inf);
    if (sf != stdout) fclose(sf);
    finish_input(o);
    return SUCCESS;
}

// --make-index: the whole input in memory, bzh_decode_index[_sync]: sized by a guess, then by what it reports.  The input is kept
int run_make_index(const Options &o)
{
    const char *doing = "error during indexing: ";
    const std::vector<uint8_t> data = read_input(o, open_input(o), doing);
    Device dev(doing);
    const size_t n = data.size();
    const uint8_t *p = n ? data.data() : &NOTHING;
    std::vector<bzh_index_entry> ent(n / 1000 + 64);
    std::vector<bzh_sync_point> pts(o.interval ? n / 8 / o.interval + 64 : 0);
    size_t count = 0, npts = 0, consumed = 0;
    uint64_t total = 0;
    auto call = [&] {
        return o.interval ? bzh_decode_index_sync(dev.ctx, p, n, o.interval, ent.data(), ent.size(), &count, pts.data(), pts.size(), &npts, &total, &consumed)
                          : bzh_decode_index(dev.ctx, p, n, ent.data(), ent.size(), &count, &total, &consumed);
    };
    auto grow = [&] { ent.resize(std::max(ent.size(), count)), pts.resize(std::max(pts.size(), npts)); };
    dev.expect(with_retry(2, call, grow));
    dev.close();
    ent.resize(count);
    pts.resize(npts);
    write_index(o.mkindex_path, ent, pts, o.interval, consumed);
    return SUCCESS;
}

// -d --index --range: the index file, the hull of the touched blocks' bytes, one bzh_decode_ranges.  The input is kept: a part of it was read
int run_range(const Options &o)
{
    const char *doing = "error during decompression: ";
    const Index ix = load_index(o.index_path, NO_RECORDS);
    const uint64_t size = regular_size(o.in_path, "--range");
    const size_t count = ix.entries.size();
    std::vector<uint32_t> touched(count);
    size_t ntouched = 0, got = 0;
    uint64_t lo = 0, hi = 0, total = 0;
    const int rs = bzh_index_spans(ix.entries.data(), count, o.ranges.data(), o.ranges.size(), touched.data(), touched.size(), &ntouched, &lo, &hi, &total);
    if (rs != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(rs));
    const std::vector<uint8_t> comp = read_span(o.in_path, size, lo, hi, doing);
    std::unique_ptr<uint8_t[]> out(new (std::nothrow) uint8_t[total ? total : 1]);
    if (!out) die(ERR_OUTPUT, std::string(doing) + "out of memory");
    if (ntouched) {
        Device dev(doing);
        std::vector<size_t> offs(o.ranges.size()), lens(o.ranges.size());
        dev.expect(bzh_decode_ranges(dev.ctx, comp.empty() ? &NOTHING : comp.data(), comp.size(), lo, ix.entries.data(), count, ix.points.data(), ix.points.size(),
                                     o.ranges.data(), o.ranges.size(), out.get(), (size_t)total, offs.data(), lens.data(), &got)); // (it failed: no output is created)
        dev.close();
    }
    write_output(open_output(output_of(o, "")), out.get(), got, doing);
    return SUCCESS;
}
// ---------------------------------------------------------------------------------------------------------------- search, grep, match
// What --search, --grep and --grep -o look through: the whole input, or with --index the bytes of the blocks the range touches
struct SearchInput {
    std::vector<uint8_t> comp;
    bool indexed = false;
    Index ix;
    uint64_t base = 0;             // where `comp` starts in the file
    bzh_range want{0, UINT64_MAX}; // the bytes of the decoded data a match must lie inside
    bool records = true;           // line numbers are known: always, but through an index that is no record index
    const uint8_t *data() const { return comp.empty() ? &NOTHING : comp.data(); }
    const uint64_t *rec_cum() const { return records ? ix.rec_cum.data() : nullptr; }
};
SearchInput load_search_input(const Options &o)
{
    const char *doing = "error during search: ";
    SearchInput in;
    if (!o.ranges.empty()) in.want = o.ranges[0];
    in.indexed = !o.index_path.empty();
    if (!in.indexed) {
        in.comp = read_input(o, open_input(o), doing);
        return in;
    }
    in.ix = load_index(o.index_path, o.grepping ? ANY_RECORDS : LINE_RECORDS);
    in.records = in.ix.is_record_index;
    const uint64_t size = regular_size(o.in_path, "--search --index");
    size_t first = 0, last = 0;
    uint64_t hi = 0;
    // (an automaton with assertions sees the byte in front of the range and the byte behind it: the widened span is read)
    const uint64_t back = in.want.off < o.look.look_behind ? in.want.off : o.look.look_behind, more = back + o.look.look_ahead;
    const int rs = bzh_index_span(in.ix.entries.data(), in.ix.entries.size(), in.want.off - back, in.want.len > UINT64_MAX - more ? UINT64_MAX : in.want.len + more,
                                  &first, &last, &in.base, &hi);
    if (rs != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(rs));
    in.comp = read_span(o.in_path, size, in.base, hi, doing, o.grepping); // (--grep walks the whole file)
    return in;
}

// The device of a search, a grep or a match, with the compiled set where there are several strings, --ignore-case, -E, -w or -x (else the
// single-pattern calls, as ever).  Up to here a failure is worded as a search's; from here on as `doing` says
Device open_search_device(const Options &o, const char *doing)
{
    Device dev("error during search: ");
    if (o.use_set) {
        const int rs = o.regex ? bzh_regex_create_ex(dev.ctx, o.pat_ptr.data(), o.pat_len.data(), o.pats.size(), o.fold(BZH_REGEX_FOLD_ASCII), 0, o.regex_flags(), &dev.set)
                               : bzh_patset_create(dev.ctx, o.pat_ptr.data(), o.pat_len.data(), o.pats.size(), o.fold(BZH_PATSET_FOLD_ASCII), &dev.set);
        if (rs != BZH_OK) dev.fail(rs, rs == BZH_E_ARG ? ERR_ARGS : ERR_OUTPUT);
        bzh_regex_info ri;
        if (o.regex && bzh_regex_get_info(dev.set, &ri) == BZH_OK && ri.unbounded)
            fprintf(stderr, "bnzhip: the expressions have matches longer than %d bytes: those are not found\n", BZH_REGEX_MAX_SPAN);
    }
    dev.doing = doing;
    return dev;
}
void flush_stdout(bool ok, const char *doing) { if (!ok || fflush(stdout) != 0) die(ERR_OUTPUT, std::string(doing) + "write failed"); }

// one search into rooms of `room` hits: of the set (shits) or of the one string (hits)
int search_call(Device &dev, const SearchInput &in, const Options &o, unsigned flags, bzh_hit *hits, bzh_set_hit *shits, size_t room, size_t *nhits)
{
    const uint8_t *pat = (const uint8_t *)o.needle.data();
    const Index &ix = in.ix;
    if (dev.set && !in.indexed) return bzh_search_patset(dev.ctx, in.data(), in.comp.size(), dev.set, flags, '\n', shits, room, nhits, nullptr, nullptr);
    if (dev.set)
        return bzh_search_patset_range(dev.ctx, in.data(), in.comp.size(), in.base, ix.entries.data(), ix.entries.size(), ix.points.data(), ix.points.size(),
                                       in.rec_cum(), in.want.off, in.want.len, dev.set, flags, '\n', shits, room, nhits);
    if (!in.indexed) return bzh_search(dev.ctx, in.data(), in.comp.size(), pat, o.needle.size(), flags, '\n', hits, room, nhits, nullptr, nullptr);
    return bzh_search_range(dev.ctx, in.data(), in.comp.size(), in.base, ix.entries.data(), ix.entries.size(), ix.points.data(), ix.points.size(), in.rec_cum(),
                            in.want.off, in.want.len, pat, o.needle.size(), flags, '\n', hits, room, nhits);
}

// --search: 'offset<TAB>line' of every occurrence ('-' for the line without a record index), with a set the string's number too
int run_search(const Options &o, const SearchInput &in)
{
    const char *doing = "error during search: ";
    Device dev = open_search_device(o, doing);
    const bool set = dev.set != nullptr;
    const unsigned flags = in.records ? BZH_SEARCH_RECORDS : 0;
    std::vector<bzh_hit> hits(o.count_only || set ? 0 : ENTRIES);
    std::vector<bzh_set_hit> shits(o.count_only || !set ? 0 : ENTRIES);
    size_t nhits = 0;
    auto call = [&] { return search_call(dev, in, o, flags, hits.data(), shits.data(), set ? shits.size() : hits.size(), &nhits); };
    dev.expect(with_retry(o.count_only ? 1 : 2, call, [&] { set ? shits.resize(nhits) : hits.resize(nhits); })); // (once more, with exactly their room)
    dev.close();
    for (size_t k = 0; k < nhits && !o.count_only; k++) {
        const unsigned long long off = set ? shits[k].off : hits[k].off, record = set ? shits[k].record : hits[k].record;
        if (in.records) printf("%llu\t%llu", off, record);
        else printf("%llu\t-", off);
        if (set) printf("\t%u\n", shits[k].pattern);
        else fputc('\n', stdout);
    }
    if (o.count_only) printf("%zu\n", nhits);
    flush_stdout(true, doing);
    return SUCCESS; // (the input is kept: nothing was made of it)
}

// one grep: the selected lines compacted into `out`, an entry a line into `lines` where they are asked for
int grep_call(Device &dev, const SearchInput &in, const Options &o, std::vector<uint8_t> &out, std::vector<bzh_grep_entry> &lines, size_t *nrecs, uint64_t *total)
{
    const unsigned flags = o.invert ? BZH_GREP_INVERT : 0;
    const uint8_t *pat = (const uint8_t *)o.needle.data(), *cp = in.data();
    uint8_t *op = out.empty() ? nullptr : out.data();
    bzh_grep_entry *lp = lines.empty() ? nullptr : lines.data();
    const Index &ix = in.ix;
    const size_t n = in.comp.size();
    if (dev.set && !in.indexed) return bzh_grep_patset(dev.ctx, cp, n, dev.set, flags, '\n', op, out.size(), lp, lines.size(), nrecs, total, nullptr, nullptr);
    if (dev.set)
        return bzh_grep_patset_index(dev.ctx, cp, n, ix.entries.data(), ix.entries.size(), ix.points.data(), ix.points.size(), dev.set, flags, '\n', op, out.size(), lp,
                                     lines.size(), nrecs, total);
    if (!in.indexed) return bzh_grep(dev.ctx, cp, n, pat, o.needle.size(), flags, '\n', op, out.size(), lp, lines.size(), nrecs, total, nullptr, nullptr);
    return bzh_grep_index(dev.ctx, cp, n, ix.entries.data(), ix.entries.size(), ix.points.data(), ix.points.size(), pat, o.needle.size(), flags, '\n', op, out.size(),
                          lp, lines.size(), nrecs, total);
}

// --grep: the selected lines as they are; with -n, -b or a context an entry a line says what to put in front and where the groups end
int run_grep(const Options &o, const SearchInput &in)
{
    const char *doing = "error during grep: ";
    Device dev = open_search_device(o, doing);
    const bool want_lines = !o.count_only && (o.line_number || o.context_given || o.byte_offset);
    std::vector<uint8_t> out(o.count_only ? 0 : CHUNK);
    std::vector<bzh_grep_entry> lines(want_lines ? ENTRIES : 0);
    if (o.context_given) bzh_grep_set_context(dev.ctx, o.ctx_before, o.ctx_after);
    size_t nrecs = 0;
    uint64_t total = 0;
    auto grow = [&] { out.resize((size_t)total), lines.resize(want_lines ? nrecs : 0); };
    dev.expect(with_retry(o.count_only ? 1 : 2, [&] { return grep_call(dev, in, o, out, lines, &nrecs, &total); }, grow));
    bzh_grep_context_stats cstats{};
    bzh_get_grep_context_stats(dev.ctx, &cstats);
    dev.close();
    bool ok = true;
    if (o.count_only) printf("%llu\n", (unsigned long long)cstats.matched); // (without a context: nrecs)
    else if (!want_lines && total) ok = fwrite(out.data(), 1, (size_t)total, stdout) == (size_t)total;
    for (size_t k = 0; want_lines && k < nrecs && ok; k++) {
        const bool is_context = (lines[k].len & BZH_GREP_LEN_CONTEXT) != 0;
        const size_t len = (size_t)(lines[k].len & ~BZH_GREP_LEN_CONTEXT);
        if (o.context_given && k && lines[k].record != lines[k - 1].record + 1) fputs("--\n", stdout);
        if (o.line_number) printf("%llu%c", (unsigned long long)lines[k].record + 1, is_context ? '-' : ':');
        if (o.byte_offset) printf("%llu%c", (unsigned long long)lines[k].off, is_context ? '-' : ':');
        ok = fwrite(out.data() + lines[k].out_off, 1, len, stdout) == len;
    }
    flush_stdout(ok, doing);
    return SUCCESS; // (the input is kept: nothing was made of it)
}

// one match: the matched parts compacted into `out`, an entry each into `ms`
int match_call(Device &dev, const SearchInput &in, const Options &o, std::vector<uint8_t> &out, std::vector<bzh_match_entry> &ms, size_t *nm, uint64_t *total)
{
    const unsigned flags = o.line_number ? BZH_MATCH_RECORDS : 0;
    const uint8_t *pat = (const uint8_t *)o.needle.data(), *cp = in.data();
    const Index &ix = in.ix;
    const size_t n = in.comp.size();
    if (dev.set && !in.indexed) return bzh_match_patset(dev.ctx, cp, n, dev.set, flags, '\n', out.data(), out.size(), ms.data(), ms.size(), nm, total, nullptr, nullptr);
    if (dev.set)
        return bzh_match_patset_index(dev.ctx, cp, n, ix.entries.data(), ix.entries.size(), ix.points.data(), ix.points.size(), dev.set, flags, '\n', out.data(),
                                      out.size(), ms.data(), ms.size(), nm, total);
    if (!in.indexed) return bzh_match(dev.ctx, cp, n, pat, o.needle.size(), flags, '\n', out.data(), out.size(), ms.data(), ms.size(), nm, total, nullptr, nullptr);
    return bzh_match_index(dev.ctx, cp, n, ix.entries.data(), ix.entries.size(), ix.points.data(), ix.points.size(), pat, o.needle.size(), flags, '\n', out.data(),
                           out.size(), ms.data(), ms.size(), nm, total);
}

// --grep -o: the matched parts alone, each on a line of its own
int run_match(const Options &o, const SearchInput &in)
{
    const char *doing = "error during grep: ";
    Device dev = open_search_device(o, doing);
    std::vector<uint8_t> out(CHUNK);
    std::vector<bzh_match_entry> ms(ENTRIES);
    size_t nm = 0;
    uint64_t total = 0;
    auto grow = [&] { out.resize(std::max<size_t>((size_t)total, 16)), ms.resize(std::max<size_t>(nm, 1)); };
    dev.expect(with_retry(2, [&] { return match_call(dev, in, o, out, ms, &nm, &total); }, grow));
    dev.close();
    bool ok = true;
    for (size_t k = 0; k < nm && ok; k++) {
        if (o.line_number) printf("%llu:", (unsigned long long)ms[k].record + 1);
        if (o.byte_offset) printf("%llu:", (unsigned long long)ms[k].off);
        ok = fwrite(out.data() + ms[k].out_off, 1, ms[k].len, stdout) == ms[k].len && fputc('\n', stdout) != EOF;
    }
    flush_stdout(ok, doing);
    return SUCCESS;
}

// --grep over several inputs: every file whole, one bzh_grep_many[_patset].  A file that cannot be read is named at once, fails alone
// and is left out of the call (the library words the first failure of a call: that text must belong to a file that was handed to it)
int run_grep_many(const Options &o)
{
    const char *doing = "error during grep: ";
    std::vector<std::string> names, paths{o.in_path};
    std::vector<std::vector<uint8_t>> many;
    bool failed = false;
    paths.insert(paths.end(), o.more_inputs.begin(), o.more_inputs.end());
    for (const std::string &path : paths) {
        std::vector<uint8_t> bytes;
        FILE *sf = fopen(path.c_str(), "rb");
        if (sf && read_all(sf, bytes)) names.push_back(path), many.push_back(std::move(bytes));
        else fprintf(stderr, "bnzhip: %s: %s\n", path.c_str(), sf ? "read failed" : strerror(errno)), failed = true;
        if (sf) fclose(sf);
    }
    Device dev = open_search_device(o, doing);
    const unsigned flags = o.invert ? BZH_GREP_INVERT : 0;
    std::vector<const uint8_t *> ins;
    std::vector<size_t> lens;
    for (const auto &m : many) ins.push_back(m.empty() ? &NOTHING : m.data()), lens.push_back(m.size());
    std::vector<uint8_t> out(o.count_only ? 0 : CHUNK);
    std::vector<bzh_grep_entry> lines(o.count_only ? 0 : ENTRIES);
    std::vector<bzh_grep_many_item> items(names.size());
    size_t nrecs = 0, e = 0;
    uint64_t total = 0;
    auto call = [&] {
        uint8_t *op = out.empty() ? nullptr : out.data();
        bzh_grep_entry *lp = lines.empty() ? nullptr : lines.data();
        if (dev.set)
            return bzh_grep_many_patset(dev.ctx, ins.data(), lens.data(), ins.size(), dev.set, flags, '\n', op, out.size(), lp, lines.size(), items.data(), &nrecs, &total);
        return bzh_grep_many(dev.ctx, ins.data(), lens.data(), ins.size(), (const uint8_t *)o.needle.data(), o.needle.size(), flags, '\n', op, out.size(), lp,
                             lines.size(), items.data(), &nrecs, &total);
    };
    auto grow = [&] { out.resize(std::max<size_t>((size_t)total, 16)), lines.resize(std::max<size_t>(nrecs, 1)); };
    dev.expect(with_retry(o.count_only ? 1 : 2, call, grow));
    const std::string first_failure = bzh_last_error(dev.ctx);
    dev.close();
    bool ok = true, worded = false;
    for (size_t k = 0; k < names.size() && ok; k++) {
        const std::string prefix = o.no_filename ? "" : names[k] + ":";
        if (items[k].status != BZH_OK) { // (the library words the first failure of a call; the others carry their status)
            fprintf(stderr, "bnzhip: %s: %s%s%s\n", names[k].c_str(), bzh_strerror(items[k].status), worded ? "" : ": ", worded ? "" : first_failure.c_str());
            failed = worded = true;
        } else if (o.count_only) {
            printf("%s%llu\n", prefix.c_str(), (unsigned long long)items[k].selected);
        }
        for (uint64_t j = 0; items[k].status == BZH_OK && !o.count_only && j < items[k].selected && ok; j++, e++) {
            const size_t len = (size_t)lines[e].len;
            fputs(prefix.c_str(), stdout);
            if (o.line_number) printf("%llu:", (unsigned long long)lines[e].record + 1);
            ok = fwrite(out.data() + lines[e].out_off, 1, len, stdout) == len;
            if (ok && len && out[lines[e].out_off + len - 1] != '\n') ok = fputc('\n', stdout) != EOF; // (a last line without its newline)
        }
    }
    flush_stdout(ok, doing);
    return failed ? ERR_OUTPUT : SUCCESS;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc <= 1) usage(false);
    Options o = parse(argc, argv);
    check(o);
    switch (o.mode) {
    case Mode::ENCODE: return run_encode(o); // (over several GPUs: run_encode_multi)
    case Mode::DECODE: return run_decode(o);
    case Mode::DECODE_STREAM: return run_decode_stream(o);
    case Mode::RECOVER: return run_recover(o);
    case Mode::MAKE_INDEX: return run_make_index(o);
    case Mode::RANGE: return run_range(o);
    case Mode::GREP_MANY: return run_grep_many(o);
    case Mode::SEARCH: return run_search(o, load_search_input(o));
    case Mode::GREP: return run_grep(o, load_search_input(o));
    case Mode::MATCH: return run_match(o, load_search_input(o));
    }
    return ERR_ARGS;
}
