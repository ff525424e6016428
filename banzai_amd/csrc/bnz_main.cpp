// bnz_main.cpp -- `bnzhip`: command-line front end over libbzhip.so with the interface of the
// reference's `bnz` (reference bnz/src/main.rs:32-59 usage, :173-257 argument grammar, :259-285 I/O
// plumbing, :292-309 keep/remove policy, :11-14 exit codes).  SURVEY.md section 8(f) row f1.
// No compression logic lives here: the input is fed to bzh_stream_feed in 16 MiB reads (like
// the reference's BufRead loop, memory stays bounded, pipes and inputs larger than memory work, and reading
// overlaps with the GPU passes) and the stream bytes are written as they become final.
// Random access: --index writes the index the streaming encoder records beside the stream (bzh_stream_begin_index),
// --make-index builds one for an existing .bz2 (bzh_decode_index_sync), -d --index --range reads byte ranges of the decoded
// data from just the compressed bytes that hold them (bzh_index_spans, bzh_decode_ranges); the files are bzh_index_blob_*'s.
// Search: --search prints the offset and the line number of every occurrence of a byte string in the decoded data, which never
// leaves the device (bzh_search; with --index bzh_search_range over just the span's compressed bytes).
// Grep: --grep writes the lines that hold a byte string, selected and compacted on the device (bzh_grep; with --index
// bzh_grep_index); with -o the matched parts alone, the non-overlapping leftmost-longest matches (bzh_match, bzh_match_index); -b
// prefixes byte offsets.  Several strings (-e, --patterns) or --ignore-case: one compiled set, one pass (bzh_patset_create, bzh_*_patset*).
// -E: the strings are regular expressions, compiled into one automaton that goes the set's way (bzh_regex_create_ex; assertions are
// always admitted).  -w, -x: the word and the line wrap of that call; without -E a string is escaped byte by byte and goes the same way.
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

[[noreturn]] void die(int code, const std::string &msg)
{
    fprintf(stderr, "%s\n", msg.c_str());
    exit(code);
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

} // namespace

int main(int argc, char **argv)
{
    if (argc <= 1) usage(false);
    enum { ANY, NOARGS, OUTPATH, IDXPATH, MKIDXPATH, INTERVAL, RANGE, SEARCH, GREP, PATTERN, PATFILE, CTX_AFTER, CTX_BEFORE, CTX_BOTH } expect = ANY;
    std::string in_path, out_path, index_path, mkindex_path, needle;
    std::vector<std::string> pats; // the strings of a set, in the order given (-e: hex with --hex; --patterns: as they stand)
    std::vector<bool> pat_hex;
    bool use_set = false, ignore_case = false, regex = false; // regex: every string is a regular expression (bzh_regex_create_ex)
    bool word_re = false, line_re = false;                    // -w, -x: the wraps of bzh_regex_create_ex; a literal string is escaped for it
    bzh_regex_look look{0, 0, 1, 0};                          // what the automaton looks at: a --range is widened by it
    auto read_patterns = [&](const std::string &path) {
        FILE *pf = fopen(path.c_str(), "rb");
        if (!pf) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + path + ": " + strerror(errno));
        std::string all;
        char buf[4096];
        for (size_t got; (got = fread(buf, 1, sizeof buf, pf)) > 0;) all.append(buf, got);
        fclose(pf);
        size_t line = 1;
        for (size_t at = 0; at < all.size(); line++) {
            size_t end = all.find('\n', at);
            if (end == std::string::npos) end = all.size();
            if (end == at) die(ERR_ARGS, "'--patterns': line " + std::to_string(line) + " of " + path + " is empty");
            pats.push_back(all.substr(at, end - at)), pat_hex.push_back(false);
            at = end + 1;
        }
    };
    bool searching = false, needle_hex = false, count_only = false;
    bool only_matching = false, byte_offset = false; // -o, -b
    bool grepping = false, invert = false, line_number = false; // (--grep is a --search that writes lines: `searching` holds for both)
    bool context_given = false; // -A, -B, -C: lines of context round every selected line
    uint32_t ctx_before = 0, ctx_after = 0;
    bool interval_given = false;
    uint32_t interval = 256;
    std::vector<bzh_range> ranges;
    // a decimal number of at most 20 digits that fits 64 bits, nothing else
    auto number = [](const std::string &t, uint64_t *v) {
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
    };
    bool have_in = false, in_stdin = false, out_stdout = false, have_out = false;
    int keep = -1, level = 9;
    bool decompress = false, recover = false, level_given = false, dstream = false;
    std::vector<std::string> more_inputs; // the inputs behind the first: --grep takes several files (judged behind the last argument)
    bool no_filename = false;
    auto set_input = [&](const std::string &p, bool is_stdin) {
        if (have_in) {
            if (is_stdin || in_stdin) die(ERR_ARGS, "Only one input may be specified");
            more_inputs.push_back(p);
            return;
        }
        have_in = true;
        in_stdin = is_stdin;
        in_path = p;
    };
    auto set_output = [&](const std::string &p, bool is_stdout) {
        if (have_out && !(out_stdout && is_stdout)) die(ERR_ARGS, "Only one output may be specified");
        have_out = true;
        out_stdout = is_stdout;
        out_path = p;
    };
    for (int k = 1; k < argc; k++) {
        const std::string a = argv[k];
        if (expect == OUTPATH) {
            if (!a.empty() && a[0] == '-') die(ERR_ARGS, "Argument '--output' requires a file path");
            set_output(a, false);
            expect = ANY;
        } else if (expect == IDXPATH || expect == MKIDXPATH) {
            const char *opt = expect == IDXPATH ? "--index" : "--make-index";
            std::string &dst = expect == IDXPATH ? index_path : mkindex_path;
            if (a.empty() || a[0] == '-') die(ERR_ARGS, std::string("Argument '") + opt + "' requires a file path");
            if (!dst.empty()) die(ERR_ARGS, std::string("'") + opt + "' may be given once");
            dst = a;
            expect = ANY;
        } else if (expect == INTERVAL) {
            uint64_t v = 0;
            if (!number(a, &v) || v > 32767) die(ERR_ARGS, "Argument '--interval' requires a number of groups, 0 to 32767");
            interval = (uint32_t)v;
            interval_given = true;
            expect = ANY;
        } else if (expect == CTX_AFTER || expect == CTX_BEFORE || expect == CTX_BOTH) {
            uint64_t v = 0;
            if (!number(a, &v) || v > UINT32_MAX) die(ERR_ARGS, "Arguments '-A', '-B' and '-C' require a number of lines, 0 to 4294967295");
            if (expect != CTX_BEFORE) ctx_after = (uint32_t)v;
            if (expect != CTX_AFTER) ctx_before = (uint32_t)v;
            context_given = true;
            expect = ANY;
        } else if (expect == RANGE) {
            const size_t colon = a.find(':');
            bzh_range r{0, 0};
            if (colon == std::string::npos || !number(a.substr(0, colon), &r.off) || !number(a.substr(colon + 1), &r.len))
                die(ERR_ARGS, "Argument '--range' requires <offset>:<length>, both in bytes");
            ranges.push_back(r);
            expect = ANY;
        } else if (expect == SEARCH || expect == GREP) {
            if (searching) die(ERR_ARGS, grepping != (expect == GREP) ? "'--grep' and '--search' exclude each other" : "'--search' and '--grep' may be given once");
            searching = true;
            grepping = expect == GREP;
            expect = ANY;
            if (a == "-e") expect = PATTERN;             // (no <string> of its own: the set's strings follow)
            else if (a == "--patterns") expect = PATFILE;
            else if (a == "--ignore-case") ignore_case = true;
            else if (a == "-E" || a == "--regex") regex = true;
            else if (a == "-w" || a == "--word-regexp") word_re = true;
            else if (a == "-x" || a == "--line-regexp") line_re = true;
            else needle = a, pats.push_back(a), pat_hex.push_back(true);
        } else if (expect == PATTERN) {
            pats.push_back(a), pat_hex.push_back(true);
            use_set = true;
            expect = ANY;
        } else if (expect == PATFILE) {
            read_patterns(a);
            use_set = true;
            expect = ANY;
        } else if (expect == ANY && a.rfind("--", 0) == 0) {
            if (a == "--help") usage(true);
            else if (a == "--version") die(SUCCESS, VERSION);
            else if (a == "--info")
                die(SUCCESS, std::string(TAGLINE) +
                                 "\n\nBlocks are suffix-sorted by prefix doubling with radix sorts, move-to-front\n"
                                 "coded and Huffman coded by HIP kernels (libbzhip.so); the stream is bit-identical\n"
                                 "to banzai 0.3.1's.\n\n" + VERSION);
            else if (a == "--verbose") {}
            else if (a == "--decompress") decompress = true;
            else if (a == "--recover") recover = true;
            else if (a == "--stream") dstream = true;
            else if (a == "--keep") keep = 1;
            else if (a == "--remove") keep = 0;
            else if (a == "--fast") level = 1, level_given = true;
            else if (a == "--best") level = 9, level_given = true;
            else if (a == "--output") expect = OUTPATH;
            else if (a == "--index") expect = IDXPATH;
            else if (a == "--make-index") expect = MKIDXPATH;
            else if (a == "--interval") expect = INTERVAL;
            else if (a == "--range") expect = RANGE;
            else if (a == "--search") expect = SEARCH;
            else if (a == "--grep") expect = GREP;
            else if (a == "--invert") invert = true;
            else if (a == "--line-number") line_number = true;
            else if (a == "--only-matching") only_matching = true;
            else if (a == "--byte-offset") byte_offset = true;
            else if (a == "--hex") needle_hex = true;
            else if (a == "--count") count_only = true;
            else if (a == "--no-filename") no_filename = true;
            else if (a == "--patterns") expect = PATFILE;
            else if (a == "--ignore-case") ignore_case = true;
            else if (a == "--regex") regex = true;
            else if (a == "--word-regexp") word_re = true;
            else if (a == "--line-regexp") line_re = true;
            else if (a == "--after-context") expect = CTX_AFTER;
            else if (a == "--before-context") expect = CTX_BEFORE;
            else if (a == "--context") expect = CTX_BOTH;
            else if (a == "--stdout") set_output("", true);
            else if (a == "--") expect = NOARGS;
            else die(ERR_ARGS, "Unrecognised argument " + a);
        } else if (expect == ANY && !a.empty() && a[0] == '-') {
            if (a == "-") {
                set_input("", true);
            } else if (a == "-e") {
                expect = PATTERN;
            } else if (a == "-E") {
                regex = true;
            } else if (a == "-w") {
                word_re = true;
            } else if (a == "-x") {
                line_re = true;
            } else if (a == "-o") {
                only_matching = true;
            } else if (a == "-b") {
                byte_offset = true;
            } else if (a == "-A") {
                expect = CTX_AFTER;
            } else if (a == "-B") {
                expect = CTX_BEFORE;
            } else if (a == "-C") {
                expect = CTX_BOTH;
            } else {
                for (size_t c = 1; c < a.size(); c++) {
                    const char f = a[c];
                    if (f == 'c') set_output("", true);
                    else if (f == 'd') decompress = true;
                    else if (f == 'k') keep = 1;
                    else if (f == 'r') keep = 0;
                    else if (f == 'v') {}
                    else if (f >= '1' && f <= '9') level = f - '0', level_given = true;
                    else die(ERR_ARGS, std::string("Flag '") + f + "' is not valid");
                }
            }
        } else {
            set_input(a, false);
        }
    }
    if (!more_inputs.empty() && !grepping) die(ERR_ARGS, "Only one input may be specified");
    if (no_filename && !grepping) die(ERR_ARGS, "'--no-filename' goes with '--grep'");
    if (!more_inputs.empty()) { // several inputs go through one bzh_grep_many: what it does not do is refused by name
        const char *opt = only_matching ? "-o" : byte_offset ? "-b" : context_given ? "-A', '-B' and '-C" : !index_path.empty() ? "--index" : nullptr;
        if (opt) die(ERR_ARGS, std::string("'") + opt + "' takes one input: several inputs go with '--grep' and '--hex', '--invert', '--count', '--line-number', '--no-filename'");
    }
    if (expect == IDXPATH || expect == MKIDXPATH) die(ERR_ARGS, "Arguments '--index' and '--make-index' require a file path");
    if (expect == INTERVAL) die(ERR_ARGS, "Argument '--interval' requires a number of groups, 0 to 32767");
    if (expect == RANGE) die(ERR_ARGS, "Argument '--range' requires <offset>:<length>, both in bytes");
    if (expect == SEARCH) die(ERR_ARGS, "Argument '--search' requires a string");
    if (expect == GREP) die(ERR_ARGS, "Argument '--grep' requires a string");
    if (expect == PATTERN) die(ERR_ARGS, "Argument '-e' requires a string");
    if (expect == CTX_AFTER || expect == CTX_BEFORE || expect == CTX_BOTH) die(ERR_ARGS, "Arguments '-A', '-B' and '-C' require a number of lines, 0 to 4294967295");
    if (expect == PATFILE) die(ERR_ARGS, "Argument '--patterns' requires a file path");
    if (word_re && line_re) die(ERR_ARGS, "'-w' and '-x' exclude each other");
    if ((word_re || line_re) && !searching) die(ERR_ARGS, "'-w' and '-x' go with '--search' or '--grep'");
    use_set = use_set || ignore_case || regex || word_re || line_re;
    if (use_set && !searching) die(ERR_ARGS, "'-e', '-E', '--patterns' and '--ignore-case' go with '--search' or '--grep'");
    if (regex && needle_hex) die(ERR_ARGS, "'-E' and '--hex' exclude each other: a regular expression writes a byte as \\xHH");
    if (use_set && pats.empty()) die(ERR_ARGS, "'--search' and '--grep' require a string, a '-e' or a '--patterns'");
    if (!have_in) die(ERR_ARGS, "An input must be specified");
    if ((needle_hex || count_only) && !searching) die(ERR_ARGS, "'--hex' and '--count' go with '--search' or '--grep'");
    if ((invert || line_number) && !grepping) die(ERR_ARGS, "'--invert' and '--line-number' go with '--grep'");
    if (context_given && !grepping) die(ERR_ARGS, "'-A', '-B' and '-C' go with '--grep'");
    if ((only_matching || byte_offset) && !grepping) die(ERR_ARGS, "'-o' and '-b' go with '--grep'");
    if (only_matching && (invert || context_given))
        die(ERR_ARGS, "'-o' writes the matched parts alone: it does not go with '--invert', '-A', '-B' or '-C'");
    if (grepping && !ranges.empty()) die(ERR_ARGS, "'--grep' takes an input, '--hex', '--invert', '--count', '--line-number', '-o', '-b', '-A', '-B', '-C' and '--index', nothing else");
    if (searching) {
        if (decompress || recover || dstream || have_out || !mkindex_path.empty() || level_given || interval_given || keep == 0)
            die(ERR_ARGS, grepping ? "'--grep' takes an input, '--hex', '--invert', '--count', '--line-number', '-o', '-b', '-A', '-B', '-C' and '--index', nothing else"
                                   : "'--search' takes an input, '--hex', '--count', '--index' and one '--range', nothing else");
        if (ranges.size() > 1 || (!ranges.empty() && index_path.empty())) die(ERR_ARGS, "'--search' takes one '--range', with the '--index' of the input");
        if (!index_path.empty() && in_stdin) die(ERR_ARGS, "'--search --index' reads parts of a file: standard in cannot be the input");
        auto unhex = [&](std::string &needle) {
            std::string raw;
            auto nib = [](char ch) { return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1; };
            if (needle.size() % 2) die(ERR_ARGS, "Argument '--search' with '--hex' requires an even number of hex digits");
            for (size_t c = 0; c < needle.size(); c += 2) {
                if (nib(needle[c]) < 0 || nib(needle[c + 1]) < 0) die(ERR_ARGS, "Argument '--search' with '--hex' requires hex digits");
                raw.push_back((char)(nib(needle[c]) * 16 + nib(needle[c + 1])));
            }
            needle = raw;
        };
        if (needle_hex && !use_set) unhex(needle);
        if (!use_set && (needle.empty() || needle.size() > BZH_SEARCH_MAX_PATTERN)) die(ERR_ARGS, "Argument '--search' requires a string of 1 to 256 bytes");
        for (size_t k = 0; use_set && k < pats.size(); k++) {
            if (needle_hex && pat_hex[k]) unhex(pats[k]);
            if (regex ? pats[k].empty() || pats[k].size() > BZH_REGEX_MAX_EXPR : pats[k].empty() || pats[k].size() > BZH_SEARCH_MAX_PATTERN)
                die(ERR_ARGS, "string " + std::to_string(k) + (regex ? " does not hold 1 to 4096 bytes" : " does not hold 1 to 256 bytes"));
        }
        if (use_set && pats.size() > BZH_PATSET_MAX_PATTERNS) die(ERR_ARGS, "more than 65536 strings");
        if ((word_re || line_re) && !regex) { // a literal string under a wrap goes the regex way, every byte as \xHH: 256 bytes become 1,024
            for (std::string &q : pats) {
                std::string esc;
                char h[8];
                for (unsigned char ch : q) snprintf(h, sizeof h, "\\x%02X", ch), esc += h;
                q = esc;
            }
            regex = true;
        }
        if (regex) { // the compile alone, on the host: what it refuses is refused before a file is read, and a --range knows its neighbours
            std::vector<const uint8_t *> pp;
            std::vector<size_t> pl;
            for (const std::string &q : pats) pp.push_back((const uint8_t *)q.data()), pl.push_back(q.size());
            char why[256] = "";
            const int rc = bzh_regex_check_ex(pp.data(), pl.data(), pp.size(), ignore_case ? BZH_REGEX_FOLD_ASCII : 0, 0,
                                              BZH_REGEX_ASSERT | (word_re ? BZH_REGEX_WORD : 0) | (line_re ? BZH_REGEX_LINE : 0), nullptr, &look, why, sizeof why);
            if (rc != BZH_OK) die(rc == BZH_E_ARG ? ERR_ARGS : ERR_OUTPUT, std::string("error during search: ") + bzh_strerror(rc) + ": " + why);
        }
    }
    const bool by_range = !ranges.empty() && !searching, make_index = !mkindex_path.empty();
    if (by_range && index_path.empty()) die(ERR_ARGS, "'--range' needs the '--index' of the input");
    if (by_range && (dstream || recover)) die(ERR_ARGS, "'--range' goes with neither '--stream' nor '--recover'");
    if (by_range && !decompress) die(ERR_ARGS, "'--range' goes with '--decompress'");
    if (by_range && in_stdin) die(ERR_ARGS, "'--range' reads parts of a file: standard in cannot be the input");
    if (by_range && !have_out) die(ERR_ARGS, "'--range' needs '--output' or '--stdout'");
    if (!index_path.empty() && !by_range && !searching && (decompress || recover)) die(ERR_ARGS, "With '--decompress' an '--index' is read by '--range'; '--recover' takes none");
    if (make_index && (decompress || recover || dstream || have_out || !index_path.empty() || level_given))
        die(ERR_ARGS, "'--make-index' takes an input, a path and '--interval', nothing else");
    if (interval_given && !make_index && (index_path.empty() || decompress)) die(ERR_ARGS, "'--interval' goes with '--make-index', or with '--index' while compressing");
    if (recover && decompress) die(ERR_ARGS, "'--recover' and '--decompress' exclude each other");
    if (dstream && recover) die(ERR_ARGS, "'--stream' and '--recover' exclude each other");
    if (dstream && !decompress) die(ERR_ARGS, "'--stream' goes with '--decompress'");
    if (recover && level_given) die(ERR_ARGS, "'--recover' takes no block size: a block is held to what the format allows");

    // a whole file -> memory (the index files, the input of --make-index)
    auto slurp = [](FILE *f, std::vector<uint8_t> &data) {
        std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)16 << 20]);
        for (;;) {
            const size_t k = fread(buf.get(), 1, (size_t)16 << 20, f);
            data.insert(data.end(), buf.get(), buf.get() + k);
            if (k < ((size_t)16 << 20)) return !ferror(f);
        }
    };
    // entries, points, interval, consumed -> an index file; -> what went wrong ("" = nothing)
    auto write_index = [](const std::string &path, const std::vector<bzh_index_entry> &ent, const std::vector<bzh_sync_point> &pts,
                          uint32_t iv, uint64_t consumed) -> std::string {
        const size_t need = bzh_index_blob_size(ent.size(), pts.size(), iv);
        std::unique_ptr<uint8_t[]> blob(need ? new (std::nothrow) uint8_t[need] : nullptr);
        size_t got = 0;
        if (!blob || bzh_index_blob_write(ent.data(), ent.size(), pts.data(), pts.size(), iv, consumed, blob.get(), need, &got) != BZH_OK)
            return "the index does not fit in memory";
        FILE *xf = fopen(path.c_str(), "wb");
        if (!xf) return "cannot create " + path + ": " + strerror(errno);
        const bool ok = fwrite(blob.get(), 1, got, xf) == got;
        if (fclose(xf) != 0 || !ok) {
            remove(path.c_str());
            return "write to " + path + " failed";
        }
        return "";
    };

    if (searching) { // --search: the whole input through bzh_search, or with --index the span of the range through bzh_search_range
        const char *doing = "error during search: ";
        const uint8_t *pat = (const uint8_t *)needle.data();
        std::vector<uint8_t> comp, blob;
        std::vector<bzh_index_entry> ent;
        std::vector<bzh_sync_point> pts;
        std::vector<uint64_t> cum;
        uint64_t lo = 0, hi = 0;
        const bzh_range want = ranges.empty() ? bzh_range{0, UINT64_MAX} : ranges[0];
        bool records = true;
        // --grep over several inputs: every file whole; one that cannot be read is named now, fails alone and is left out of the call
        // (the library words the first failure of a call: that text must belong to a file that was handed to it)
        std::vector<std::string> names;
        std::vector<std::vector<uint8_t>> many;
        const bool several = !more_inputs.empty();
        bool unread = false;
        if (several) {
            std::vector<std::string> paths{in_path};
            paths.insert(paths.end(), more_inputs.begin(), more_inputs.end());
            for (const std::string &path : paths) {
                std::vector<uint8_t> bytes;
                FILE *sf = fopen(path.c_str(), "rb");
                if (!sf || !slurp(sf, bytes)) {
                    fprintf(stderr, "bnzhip: %s: %s\n", path.c_str(), sf ? "read failed" : strerror(errno));
                    unread = true;
                } else {
                    names.push_back(path), many.push_back(std::move(bytes));
                }
                if (sf) fclose(sf);
            }
        } else if (!index_path.empty()) {
            FILE *xf = fopen(index_path.c_str(), "rb");
            if (!xf) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + index_path + ": " + strerror(errno));
            const bool xok = slurp(xf, blob);
            fclose(xf);
            if (!xok) die(ERR_FILESYSTEM, "[filesystem error] cannot read " + index_path);
            const std::string damaged = "[filesystem error] " + index_path + " is not a whole, undamaged index file";
            // a record index ("BZhREC\r\n" | u32 version 1 | u32 delim | u64 entries | u64 records | u32 CRC-32 | u32 0 | an index blob | the
            // table of entries + 1 words): the blob inside it and the table; else a block or sync index, and no line numbers
            const uint8_t *ib = blob.data();
            size_t in = blob.size();
            auto get = [&](size_t at, int bytes) {
                uint64_t v = 0;
                for (int j = bytes - 1; j >= 0; j--) v = v << 8 | blob[at + j];
                return v;
            };
            records = blob.size() >= 40 && memcmp(blob.data(), "BZhREC\r\n", 8) == 0;
            if (records) {
                const uint64_t nent = get(16, 8);
                if (get(8, 4) != 1 || get(36, 4) != 0 || nent >= blob.size() / 8 || blob.size() < 40 + 8 * (nent + 1)) die(ERR_FILESYSTEM, damaged);
                uint32_t crc = 0xFFFFFFFFu; // zlib's CRC-32 over the header with its CRC field zero and everything behind it
                for (size_t at = 0; at < blob.size(); at++) {
                    crc ^= at >= 32 && at < 36 ? 0u : blob[at];
                    for (int j = 0; j < 8; j++) crc = crc >> 1 ^ (0xEDB88320u & (0u - (crc & 1u)));
                }
                if ((crc ^ 0xFFFFFFFFu) != (uint32_t)get(32, 4)) die(ERR_FILESYSTEM, damaged);
                if (get(12, 4) != '\n' && !grepping) die(ERR_ARGS, "'--search' counts lines: " + index_path + " holds records of another delimiter");
                cum.resize((size_t)nent + 1);
                for (size_t e = 0; e <= nent; e++) cum[e] = get(blob.size() - 8 * (nent + 1) + 8 * e, 8);
                ib = blob.data() + 40;
                in = blob.size() - 40 - 8 * ((size_t)nent + 1);
            }
            static const uint8_t none = 0;
            size_t count = 0, npts = 0;
            uint32_t iv = 0;
            uint64_t consumed = 0;
            int rs = bzh_index_blob_read(in ? ib : &none, in, nullptr, 0, &count, nullptr, 0, &npts, &iv, &consumed);
            ent.resize(count), pts.resize(npts);
            if (rs == BZH_E_CAP) rs = bzh_index_blob_read(ib, in, ent.data(), count, &count, pts.data(), npts, &npts, &iv, &consumed);
            if (rs != BZH_OK || (records && cum.size() != count + 1)) die(ERR_FILESYSTEM, damaged);
            struct stat sb;
            if (stat(in_path.c_str(), &sb) != 0) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + in_path + ": " + strerror(errno));
            if (!S_ISREG(sb.st_mode)) die(ERR_ARGS, "'--search --index' reads parts of a regular file: " + in_path + " is none");
            size_t first = 0, last = 0;
            // (an automaton with assertions sees the byte in front of the range and the byte behind it: the widened span is read)
            const uint64_t back = want.off < look.look_behind ? want.off : look.look_behind, more = back + look.look_ahead;
            rs = bzh_index_span(ent.data(), count, want.off - back, want.len > UINT64_MAX - more ? UINT64_MAX : want.len + more, &first, &last, &lo, &hi);
            if (rs != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(rs));
            if (hi < lo || hi > (uint64_t)sb.st_size)
                die(ERR_OUTPUT, std::string(doing) + "the index names bytes behind the end of " + in_path + ": it is not this file's");
            FILE *rf = fopen(in_path.c_str(), "rb");
            if (!rf) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + in_path + ": " + strerror(errno));
            if (grepping) lo = 0, hi = (uint64_t)sb.st_size; // (the whole file is walked)
            comp.resize((size_t)(hi - lo));
            if (!comp.empty() && (fseeko(rf, (off_t)lo, SEEK_SET) != 0 || fread(comp.data(), 1, comp.size(), rf) != comp.size()))
                die(ERR_OUTPUT, std::string(doing) + "read failed");
            fclose(rf);
        } else {
            FILE *sf = in_stdin ? stdin : fopen(in_path.c_str(), "rb");
            if (!sf) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + in_path + ": " + strerror(errno));
            if (!slurp(sf, comp)) die(ERR_OUTPUT, std::string(doing) + "read failed");
            if (sf != stdin) fclose(sf);
        }
        const char *dv = getenv("BZHIP_DEVICE");
        bzh_ctx *sctx = nullptr;
        int rs = bzh_create(&sctx, dv ? atoi(dv) : 0, 9, 0);
        if (rs != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(rs));
        static const uint8_t nothing = 0;
        const uint8_t *cp = comp.empty() ? &nothing : comp.data();
        bzh_patset *set = nullptr; // several strings or --ignore-case: one compiled set; else the single-pattern calls, as ever
        if (use_set) {
            std::vector<const uint8_t *> pp;
            std::vector<size_t> pl;
            for (const std::string &q : pats) pp.push_back((const uint8_t *)q.data()), pl.push_back(q.size());
            if (regex)
                rs = bzh_regex_create_ex(sctx, pp.data(), pl.data(), pp.size(), ignore_case ? BZH_REGEX_FOLD_ASCII : 0, 0,
                                         BZH_REGEX_ASSERT | (word_re ? BZH_REGEX_WORD : 0) | (line_re ? BZH_REGEX_LINE : 0), &set);
            else rs = bzh_patset_create(sctx, pp.data(), pl.data(), pp.size(), ignore_case ? BZH_PATSET_FOLD_ASCII : 0, &set);
            if (rs != BZH_OK) {
                const std::string msg = std::string(doing) + bzh_strerror(rs) + ": " + bzh_last_error(sctx);
                bzh_destroy(sctx);
                die(rs == BZH_E_ARG ? ERR_ARGS : ERR_OUTPUT, msg);
            }
            bzh_regex_info ri;
            if (regex && bzh_regex_get_info(set, &ri) == BZH_OK && ri.unbounded)
                fprintf(stderr, "bnzhip: the expressions have matches longer than %d bytes: those are not found\n", BZH_REGEX_MAX_SPAN);
        }
        if (several) { // --grep over several inputs: one bzh_grep_many; a first try with a guess, a second with the exact rooms
            const unsigned gflags = invert ? BZH_GREP_INVERT : 0;
            std::vector<const uint8_t *> ins;
            std::vector<size_t> lens;
            for (const auto &m : many) ins.push_back(m.empty() ? &nothing : m.data()), lens.push_back(m.size());
            std::vector<uint8_t> out(count_only ? 0 : (size_t)16 << 20);
            std::vector<bzh_grep_entry> lines(count_only ? 0 : (size_t)1 << 16);
            std::vector<bzh_grep_many_item> items(names.size());
            size_t nrecs = 0;
            uint64_t total = 0;
            for (int attempt = 0; attempt < 2; attempt++) {
                uint8_t *op = out.empty() ? nullptr : out.data();
                bzh_grep_entry *lp = lines.empty() ? nullptr : lines.data();
                if (set)
                    rs = bzh_grep_many_patset(sctx, ins.data(), lens.data(), ins.size(), set, gflags, '\n', op, out.size(), lp, lines.size(), items.data(),
                                              &nrecs, &total);
                else
                    rs = bzh_grep_many(sctx, ins.data(), lens.data(), ins.size(), pat, needle.size(), gflags, '\n', op, out.size(), lp, lines.size(),
                                       items.data(), &nrecs, &total);
                if (rs != BZH_E_CAP || count_only || attempt) break;
                out.resize(std::max<size_t>((size_t)total, 16));
                lines.resize(std::max<size_t>(nrecs, 1));
            }
            const std::string msg = rs == BZH_OK ? "" : std::string("error during grep: ") + bzh_strerror(rs) + ": " + bzh_last_error(sctx);
            const std::string first_failure = bzh_last_error(sctx);
            bzh_patset_destroy(set);
            bzh_destroy(sctx);
            if (rs != BZH_OK) die(ERR_OUTPUT, msg);
            bool ok = true, failed = unread, worded = false;
            size_t e = 0;
            for (size_t k = 0; k < names.size() && ok; k++) {
                const std::string prefix = no_filename ? "" : names[k] + ":";
                if (items[k].status != BZH_OK) { // (the library words the first failure of a call; the others carry their status)
                    failed = true;
                    fprintf(stderr, "bnzhip: %s: %s%s%s\n", names[k].c_str(), bzh_strerror(items[k].status), worded ? "" : ": ", worded ? "" : first_failure.c_str());
                    worded = true;
                    continue;
                }
                if (count_only) {
                    printf("%s%llu\n", prefix.c_str(), (unsigned long long)items[k].selected);
                    continue;
                }
                for (uint64_t j = 0; j < items[k].selected && ok; j++, e++) {
                    const size_t len = (size_t)lines[e].len;
                    fputs(prefix.c_str(), stdout);
                    if (line_number) printf("%llu:", (unsigned long long)lines[e].record + 1);
                    ok = fwrite(out.data() + lines[e].out_off, 1, len, stdout) == len;
                    if (ok && len && out[lines[e].out_off + len - 1] != '\n') ok = fputc('\n', stdout) != EOF; // (a last line without its newline)
                }
            }
            if (!ok || fflush(stdout) != 0) die(ERR_OUTPUT, "error during grep: write failed");
            return failed ? ERR_OUTPUT : SUCCESS;
        }
        if (grepping && only_matching && !count_only) { // --grep -o: the matched parts come back compacted, an entry each
            const unsigned mflags = line_number ? BZH_MATCH_RECORDS : 0;
            std::vector<uint8_t> out((size_t)16 << 20);
            std::vector<bzh_match_entry> ms((size_t)1 << 16);
            size_t nm = 0;
            uint64_t total = 0;
            for (int attempt = 0; attempt < 2; attempt++) {
                if (set && index_path.empty())
                    rs = bzh_match_patset(sctx, cp, comp.size(), set, mflags, '\n', out.data(), out.size(), ms.data(), ms.size(), &nm, &total, nullptr, nullptr);
                else if (set)
                    rs = bzh_match_patset_index(sctx, cp, comp.size(), ent.data(), ent.size(), pts.data(), pts.size(), set, mflags, '\n', out.data(),
                                                out.size(), ms.data(), ms.size(), &nm, &total);
                else if (index_path.empty())
                    rs = bzh_match(sctx, cp, comp.size(), pat, needle.size(), mflags, '\n', out.data(), out.size(), ms.data(), ms.size(), &nm, &total,
                                   nullptr, nullptr);
                else
                    rs = bzh_match_index(sctx, cp, comp.size(), ent.data(), ent.size(), pts.data(), pts.size(), pat, needle.size(), mflags, '\n',
                                         out.data(), out.size(), ms.data(), ms.size(), &nm, &total);
                if (rs != BZH_E_CAP || attempt) break;
                out.resize(std::max<size_t>((size_t)total, 16));
                ms.resize(std::max<size_t>(nm, 1));
            }
            const std::string msg = rs == BZH_OK ? "" : std::string("error during grep: ") + bzh_strerror(rs) + ": " + bzh_last_error(sctx);
            bzh_patset_destroy(set);
            bzh_destroy(sctx);
            if (rs != BZH_OK) die(ERR_OUTPUT, msg);
            bool ok = true;
            for (size_t k = 0; k < nm && ok; k++) {
                if (line_number) printf("%llu:", (unsigned long long)ms[k].record + 1);
                if (byte_offset) printf("%llu:", (unsigned long long)ms[k].off);
                ok = fwrite(out.data() + ms[k].out_off, 1, ms[k].len, stdout) == ms[k].len && fputc('\n', stdout) != EOF;
            }
            if (!ok || fflush(stdout) != 0) die(ERR_OUTPUT, "error during grep: write failed");
            return SUCCESS;
        }
        if (grepping) { // --grep: the selected lines come back compacted; a first try with a guess, a second with the exact rooms
            const unsigned gflags = invert ? BZH_GREP_INVERT : 0;
            std::vector<uint8_t> out(count_only ? 0 : (size_t)16 << 20);
            const bool want_lines = !count_only && (line_number || context_given || byte_offset); // (with context: where the groups end)
            std::vector<bzh_grep_entry> lines(want_lines ? (size_t)1 << 16 : 0);
            if (context_given) bzh_grep_set_context(sctx, ctx_before, ctx_after);
            size_t nrecs = 0;
            uint64_t total = 0;
            for (int attempt = 0; attempt < 2; attempt++) {
                uint8_t *op = out.empty() ? nullptr : out.data();
                bzh_grep_entry *lp = lines.empty() ? nullptr : lines.data();
                if (set && index_path.empty())
                    rs = bzh_grep_patset(sctx, cp, comp.size(), set, gflags, '\n', op, out.size(), lp, lines.size(), &nrecs, &total, nullptr, nullptr);
                else if (set)
                    rs = bzh_grep_patset_index(sctx, cp, comp.size(), ent.data(), ent.size(), pts.data(), pts.size(), set, gflags, '\n', op, out.size(),
                                               lp, lines.size(), &nrecs, &total);
                else if (index_path.empty())
                    rs = bzh_grep(sctx, cp, comp.size(), pat, needle.size(), gflags, '\n', op, out.size(), lp, lines.size(), &nrecs, &total, nullptr,
                                  nullptr);
                else
                    rs = bzh_grep_index(sctx, cp, comp.size(), ent.data(), ent.size(), pts.data(), pts.size(), pat, needle.size(), gflags, '\n', op,
                                        out.size(), lp, lines.size(), &nrecs, &total);
                if (rs != BZH_E_CAP || count_only || attempt) break;
                out.resize((size_t)total);
                if (want_lines) lines.resize(nrecs);
            }
            bzh_grep_context_stats cstats{};
            if (rs == BZH_OK) bzh_get_grep_context_stats(sctx, &cstats);
            if (rs != BZH_OK) {
                const std::string msg = std::string("error during grep: ") + bzh_strerror(rs) + ": " + bzh_last_error(sctx);
                bzh_patset_destroy(set);
                bzh_destroy(sctx);
                die(ERR_OUTPUT, msg);
            }
            bzh_patset_destroy(set);
            bzh_destroy(sctx);
            bool ok = true;
            if (count_only) {
                printf("%llu\n", (unsigned long long)cstats.matched); // (without a context: nrecs)
            } else if (want_lines) {
                for (size_t k = 0; k < nrecs && ok; k++) {
                    const bool is_context = (lines[k].len & BZH_GREP_LEN_CONTEXT) != 0;
                    const size_t len = (size_t)(lines[k].len & ~BZH_GREP_LEN_CONTEXT);
                    if (context_given && k && lines[k].record != lines[k - 1].record + 1) fputs("--\n", stdout);
                    if (line_number) printf("%llu%c", (unsigned long long)lines[k].record + 1, is_context ? '-' : ':');
                    if (byte_offset) printf("%llu%c", (unsigned long long)lines[k].off, is_context ? '-' : ':');
                    ok = fwrite(out.data() + lines[k].out_off, 1, len, stdout) == len;
                }
            } else if (total) {
                ok = fwrite(out.data(), 1, (size_t)total, stdout) == (size_t)total;
            }
            if (!ok || fflush(stdout) != 0) die(ERR_OUTPUT, "error during grep: write failed");
            return SUCCESS; // (the input is kept: nothing was made of it)
        }
        const unsigned flags = records ? BZH_SEARCH_RECORDS : 0;
        std::vector<bzh_hit> hits(count_only || set ? 0 : (size_t)1 << 16);
        std::vector<bzh_set_hit> shits(count_only || !set ? 0 : (size_t)1 << 16);
        size_t nhits = 0;
        for (int attempt = 0; attempt < 2; attempt++) { // (more hits than the first try's room: once more, with exactly theirs)
            if (set && index_path.empty())
                rs = bzh_search_patset(sctx, cp, comp.size(), set, flags, '\n', shits.data(), shits.size(), &nhits, nullptr, nullptr);
            else if (set)
                rs = bzh_search_patset_range(sctx, cp, comp.size(), lo, ent.data(), ent.size(), pts.data(), pts.size(), records ? cum.data() : nullptr,
                                             want.off, want.len, set, flags, '\n', shits.data(), shits.size(), &nhits);
            else if (index_path.empty())
                rs = bzh_search(sctx, cp, comp.size(), pat, needle.size(), flags, '\n', hits.data(), hits.size(), &nhits, nullptr, nullptr);
            else
                rs = bzh_search_range(sctx, cp, comp.size(), lo, ent.data(), ent.size(), pts.data(), pts.size(), records ? cum.data() : nullptr,
                                      want.off, want.len, pat, needle.size(), flags, '\n', hits.data(), hits.size(), &nhits);
            if (rs != BZH_E_CAP || count_only || attempt) break;
            if (set) shits.resize(nhits);
            else hits.resize(nhits);
        }
        if (rs != BZH_OK) {
            const std::string msg = std::string(doing) + bzh_strerror(rs) + ": " + bzh_last_error(sctx);
            bzh_patset_destroy(set);
            bzh_destroy(sctx);
            die(ERR_OUTPUT, msg);
        }
        bzh_patset_destroy(set);
        bzh_destroy(sctx);
        if (count_only) {
            printf("%zu\n", nhits);
        } else if (set) {
            for (size_t k = 0; k < nhits; k++) {
                if (records)
                    printf("%llu\t%llu\t%u\n", (unsigned long long)shits[k].off, (unsigned long long)shits[k].record, shits[k].pattern);
                else
                    printf("%llu\t-\t%u\n", (unsigned long long)shits[k].off, shits[k].pattern);
            }
        } else {
            for (size_t k = 0; k < nhits; k++) {
                if (records)
                    printf("%llu\t%llu\n", (unsigned long long)hits[k].off, (unsigned long long)hits[k].record);
                else
                    printf("%llu\t-\n", (unsigned long long)hits[k].off);
            }
        }
        if (fflush(stdout) != 0) die(ERR_OUTPUT, std::string(doing) + "write failed");
        return SUCCESS; // (the input is kept: nothing was made of it)
    }

    if (by_range) { // -d --index --range: the index file, the hull of the touched blocks' bytes, one bzh_decode_ranges
        const char *doing = "error during decompression: ";
        std::vector<uint8_t> blob;
        FILE *xf = fopen(index_path.c_str(), "rb");
        if (!xf) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + index_path + ": " + strerror(errno));
        const bool xok = slurp(xf, blob);
        fclose(xf);
        if (!xok) die(ERR_FILESYSTEM, "[filesystem error] cannot read " + index_path);
        static const uint8_t none = 0;
        size_t count = 0, npts = 0;
        uint32_t iv = 0;
        uint64_t consumed = 0;
        int rs = bzh_index_blob_read(blob.empty() ? &none : blob.data(), blob.size(), nullptr, 0, &count, nullptr, 0, &npts, &iv, &consumed);
        std::vector<bzh_index_entry> ent(count);
        std::vector<bzh_sync_point> pts(npts);
        if (rs == BZH_E_CAP) rs = bzh_index_blob_read(blob.data(), blob.size(), ent.data(), count, &count, pts.data(), npts, &npts, &iv, &consumed);
        if (rs != BZH_OK) die(ERR_FILESYSTEM, "[filesystem error] " + index_path + " is not a whole, undamaged index file");
        blob = std::vector<uint8_t>();
        struct stat sb;
        if (stat(in_path.c_str(), &sb) != 0) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + in_path + ": " + strerror(errno));
        if (!S_ISREG(sb.st_mode)) die(ERR_ARGS, "'--range' reads parts of a regular file: " + in_path + " is none");
        FILE *rf = fopen(in_path.c_str(), "rb");
        if (!rf) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + in_path + ": " + strerror(errno));
        std::vector<uint32_t> touched(count);
        size_t ntouched = 0;
        uint64_t lo = 0, hi = 0, total = 0;
        rs = bzh_index_spans(ent.data(), count, ranges.data(), ranges.size(), touched.data(), touched.size(), &ntouched, &lo, &hi, &total);
        if (rs != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(rs));
        if (hi < lo || hi > (uint64_t)sb.st_size) // (before anything is sized by them)
            die(ERR_OUTPUT, std::string(doing) + "the index names bytes behind the end of " + in_path + ": it is not this file's");
        const size_t span = (size_t)(hi - lo);
        std::unique_ptr<uint8_t[]> comp(new (std::nothrow) uint8_t[span ? span : 1]), out(new (std::nothrow) uint8_t[total ? total : 1]);
        if (!comp || !out) die(ERR_OUTPUT, std::string(doing) + "out of memory");
        if (span) {
            if (fseeko(rf, (off_t)lo, SEEK_SET) != 0 || fread(comp.get(), 1, span, rf) != span) die(ERR_OUTPUT, std::string(doing) + "read failed");
        }
        fclose(rf);
        size_t got = 0;
        if (ntouched) {
            const char *dv = getenv("BZHIP_DEVICE");
            bzh_ctx *rctx = nullptr;
            rs = bzh_create(&rctx, dv ? atoi(dv) : 0, 9, 0);
            if (rs != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(rs));
            std::vector<size_t> offs(ranges.size()), lens(ranges.size());
            rs = bzh_decode_ranges(rctx, comp.get(), span, lo, ent.data(), count, pts.data(), npts, ranges.data(), ranges.size(), out.get(),
                                   (size_t)total, offs.data(), lens.data(), &got);
            if (rs != BZH_OK) { // (no output is created)
                const std::string msg = std::string(doing) + bzh_strerror(rs) + ": " + bzh_last_error(rctx);
                bzh_destroy(rctx);
                die(ERR_OUTPUT, msg);
            }
            bzh_destroy(rctx);
        }
        FILE *df = stdout;
        if (!out_stdout) {
            df = fopen(out_path.c_str(), "wb");
            if (!df) die(ERR_FILESYSTEM, "[filesystem error] cannot create " + out_path + ": " + strerror(errno));
        }
        if (got && fwrite(out.get(), 1, got, df) != got) die(ERR_OUTPUT, std::string(doing) + "write failed");
        if (fflush(df) != 0) die(ERR_OUTPUT, std::string(doing) + "write failed");
        if (df != stdout) fclose(df);
        return SUCCESS; // (the input is kept: a part of it was read)
    }

    FILE *inf = in_stdin ? stdin : fopen(in_path.c_str(), "rb");
    if (!inf) die(ERR_FILESYSTEM, "[filesystem error] cannot open " + in_path + ": " + strerror(errno));

    if (make_index) { // the whole input in memory, a level-9 context, bzh_decode_index[_sync]: sized by a guess, then by what it reports
        const char *doing = "error during indexing: ";
        std::vector<uint8_t> data;
        if (!slurp(inf, data)) die(ERR_OUTPUT, std::string(doing) + "read failed");
        if (!in_stdin) fclose(inf);
        const char *dv = getenv("BZHIP_DEVICE");
        bzh_ctx *xctx = nullptr;
        int xs = bzh_create(&xctx, dv ? atoi(dv) : 0, 9, 0);
        if (xs != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(xs));
        static const uint8_t none = 0;
        const size_t n = data.size();
        std::vector<bzh_index_entry> ent(n / 1000 + 64);
        std::vector<bzh_sync_point> pts(interval ? n / 8 / interval + 64 : 0);
        size_t count = 0, npts = 0, consumed = 0;
        uint64_t total = 0;
        for (int attempt = 0; attempt < 2; attempt++) {
            xs = interval ? bzh_decode_index_sync(xctx, n ? data.data() : &none, n, interval, ent.data(), ent.size(), &count, pts.data(),
                                                  pts.size(), &npts, &total, &consumed)
                          : bzh_decode_index(xctx, n ? data.data() : &none, n, ent.data(), ent.size(), &count, &total, &consumed);
            if (xs != BZH_E_CAP) break;
            if (count > ent.size()) ent.resize(count);
            if (npts > pts.size()) pts.resize(npts);
        }
        if (xs != BZH_OK) {
            const std::string msg = std::string(doing) + bzh_strerror(xs) + ": " + bzh_last_error(xctx);
            bzh_destroy(xctx);
            die(ERR_OUTPUT, msg);
        }
        bzh_destroy(xctx);
        ent.resize(count);
        pts.resize(npts);
        const std::string bad = write_index(mkindex_path, ent, pts, interval, consumed);
        if (!bad.empty()) die(ERR_FILESYSTEM, "[filesystem error] " + bad);
        return SUCCESS; // (the input is kept)
    }

    if (decompress || recover) { // the whole input in memory, a level-9 context, one call (more where a size guess was short); --stream: neither
        const char *doing = recover ? "error during recovery: " : "error during decompression: ";
        std::string dpath = out_path;
        if (!have_out && !in_stdin) {
            if (in_path.size() < 5 || in_path.compare(in_path.size() - 4, 4, ".bz2") != 0)
                die(ERR_ARGS, std::string("With ") + (recover ? "--recover" : "--decompress") +
                                  " the input path must end in '.bz2' unless --output or --stdout is given");
            dpath = in_path.substr(0, in_path.size() - 4);
        }
        if (dstream) { // bzh_dstream_feed through two fixed buffers: 8 MiB reads, 16 MiB writes
            const bool to_file = !(have_out && out_stdout) && !(in_stdin && !have_out);
            const char *sv = getenv("BZHIP_DEVICE");
            bzh_ctx *sctx = nullptr;
            int ss = bzh_create(&sctx, sv ? atoi(sv) : 0, 9, 0);
            if (ss != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(ss));
            FILE *sf = stdout;
            auto sfail = [&](const std::string &what) { // no partial output file is left behind
                const std::string msg = std::string(doing) + what;
                bzh_destroy(sctx);
                if (sf != stdout) {
                    fclose(sf);
                    remove(dpath.c_str());
                }
                die(ERR_OUTPUT, msg);
            };
            ss = bzh_dstream_begin(sctx);
            if (ss != BZH_OK) sfail(std::string(bzh_strerror(ss)) + ": " + bzh_last_error(sctx));
            if (to_file) {
                sf = fopen(dpath.c_str(), "wb");
                if (!sf) {
                    bzh_destroy(sctx);
                    die(ERR_FILESYSTEM, "[filesystem error] cannot create " + dpath + ": " + strerror(errno));
                }
            }
            const size_t IN_CHUNK = (size_t)8 << 20, OUT_CHUNK = (size_t)16 << 20;
            std::unique_ptr<uint8_t[]> ibuf(new uint8_t[IN_CHUNK]), obuf(new uint8_t[OUT_CHUNK]);
            int done = 0;
            for (bool eof = false; !done;) {
                size_t k = 0;
                if (!eof) {
                    k = fread(ibuf.get(), 1, IN_CHUNK, inf);
                    if (k < IN_CHUNK) {
                        if (ferror(inf)) sfail("read failed");
                        eof = true;
                    }
                }
                for (size_t off = 0;;) { // until the chunk is used and nothing more comes out
                    size_t used = 0, got = 0;
                    ss = bzh_dstream_feed(sctx, ibuf.get() + off, k - off, eof ? 1 : 0, &used, obuf.get(), OUT_CHUNK, &got, &done);
                    if (ss != BZH_OK) sfail(std::string(bzh_strerror(ss)) + ": " + bzh_last_error(sctx));
                    if (got && fwrite(obuf.get(), 1, got, sf) != got) sfail("write failed");
                    off += used;
                    if (done || (off == k && got < OUT_CHUNK && !eof)) break;
                }
            }
            bzh_destroy(sctx);
            sctx = nullptr;
            if (!in_stdin) fclose(inf);
            if (fflush(sf) != 0) {
                if (sf != stdout) fclose(sf), remove(dpath.c_str());
                die(ERR_OUTPUT, std::string(doing) + "write failed");
            }
            if (sf != stdout) fclose(sf);
            const bool keep_in = keep >= 0 ? keep == 1 : have_out; // bnz/src/main.rs:292-300
            if (!keep_in && !in_stdin && remove(in_path.c_str()) != 0)
                die(ERR_OUTPUT, "error deleting input file: " + std::string(strerror(errno)));
            return SUCCESS;
        }
        std::vector<uint8_t> data;
        {
            std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)16 << 20]);
            for (;;) {
                const size_t k = fread(buf.get(), 1, (size_t)16 << 20, inf);
                data.insert(data.end(), buf.get(), buf.get() + k);
                if (k < ((size_t)16 << 20)) {
                    if (ferror(inf)) die(ERR_OUTPUT, std::string(doing) + "read failed");
                    break;
                }
            }
        }
        if (!in_stdin) fclose(inf);
        const char *dv = getenv("BZHIP_DEVICE");
        bzh_ctx *dctx = nullptr;
        int ds = bzh_create(&dctx, dv ? atoi(dv) : 0, 9, 0);
        if (ds != BZH_OK) die(ERR_OUTPUT, std::string(doing) + bzh_strerror(ds));
        static const uint8_t none = 0;
        const size_t n = data.size();
        size_t cap = 6 * n + 65536, got = 0;
        std::unique_ptr<uint8_t[]> out;
        size_t lost = 0;
        if (recover) { // one bzh_recover with a guessed room for the bytes and for the report; BZH_E_CAP names what either needs
            size_t count = 0, kept = 0;
            std::vector<bzh_recover_entry> ent(n / 1000 + 64);
            for (int attempt = 0; attempt < 3; attempt++) {
                out.reset(new (std::nothrow) uint8_t[cap ? cap : 1]);
                ds = out ? bzh_recover(dctx, n ? data.data() : &none, n, out.get(), cap, &got, ent.data(), ent.size(), &count) : BZH_E_NOMEM;
                if (ds != BZH_E_CAP) break;
                if (got > cap) cap = got;
                if (count > ent.size()) ent.resize(count);
            }
            bzh_recover_stats rs{};
            if (ds == BZH_OK) ds = bzh_get_recover_stats(dctx, &rs);
            if (ds == BZH_OK) {
                for (size_t k = 0; k < count; k++) {
                    const bzh_recover_entry &e = ent[k];
                    if (e.kind == 0) {
                        kept++;
                        continue;
                    }
                    lost++;
                    const char *why = e.kind == BZH_LOST_TRUNC ? "truncated" : e.kind == BZH_LOST_FORMAT ? "field outside the format"
                                    : e.kind == BZH_LOST_BLOCK_CRC ? "block CRC mismatch" : e.kind == BZH_LOST_RANDOMISED ? "randomised block" : "error";
                    fprintf(stderr, "lost: block at bit %llu: %s (found at bit %llu)\n", (unsigned long long)e.bit_pos, why,
                            (unsigned long long)e.err_bit);
                }
                fprintf(stderr, "recovered: %zu blocks kept, %zu lost, %zu bytes, %llu streams whole\n", kept, lost, got,
                        (unsigned long long)rs.streams_ok);
            }
        } else { // one bzh_decode, a second one if the first size guess was short
            for (int attempt = 0; attempt < 2; attempt++) {
                out.reset(new (std::nothrow) uint8_t[cap ? cap : 1]);
                ds = out ? bzh_decode(dctx, n ? data.data() : &none, n, out.get(), cap, &got, nullptr) : BZH_E_NOMEM;
                if (ds != BZH_E_CAP) break;
                cap = got; // the size the library reports
            }
        }
        if (ds != BZH_OK) { // the input stays where it is, and no output is created
            const std::string msg = std::string(doing) + bzh_strerror(ds) + ": " + bzh_last_error(dctx);
            bzh_destroy(dctx);
            die(ERR_OUTPUT, msg);
        }
        bzh_destroy(dctx); // (both ways out below leave nothing open)
        FILE *df = stdout;
        if (!(have_out && out_stdout) && !(in_stdin && !have_out)) {
            df = fopen(dpath.c_str(), "wb");
            if (!df) die(ERR_FILESYSTEM, "[filesystem error] cannot create " + dpath + ": " + strerror(errno));
        }
        if (got && fwrite(out.get(), 1, got, df) != got) die(ERR_OUTPUT, std::string(doing) + "write failed");
        if (fflush(df) != 0) die(ERR_OUTPUT, std::string(doing) + "write failed");
        if (df != stdout) fclose(df);
        if (lost) return LOST_BLOCKS; // (a damaged archive of which blocks were lost is never removed)
        const bool keep_in = keep >= 0 ? keep == 1 : have_out; // bnz/src/main.rs:292-300
        if (!keep_in && !in_stdin && remove(in_path.c_str()) != 0)
            die(ERR_OUTPUT, "error deleting input file: " + std::string(strerror(errno)));
        return SUCCESS;
    }

    FILE *outf = stdout;
    if (have_out && !out_stdout) {
        outf = fopen(out_path.c_str(), "wb");
        if (!outf) die(ERR_FILESYSTEM, "[filesystem error] cannot create " + out_path + ": " + strerror(errno));
    } else if (!have_out && !in_stdin) {
        const std::string p = in_path + ".bz2";
        outf = fopen(p.c_str(), "wb");
        if (!outf) die(ERR_FILESYSTEM, "[filesystem error] cannot create " + p + ": " + strerror(errno));
    }

    // $BZHIP_DEVICES = "0,1,2,3": the GPUs of this node the blocks are spread over (bzh_create_multi: one host thread and
    // context per device inside the library; the stream is the one a single device writes).  That path holds the whole
    // input in memory; with one device (the default) the input is streamed as below.
    if (const char *dl = getenv("BZHIP_DEVICES")) {
        std::vector<int> devices;
        for (const char *q = dl; *q;) {
            char *e = nullptr;
            const long v = strtol(q, &e, 10);
            if (e == q) break;
            devices.push_back((int)v);
            q = *e == ',' ? e + 1 : e;
            if (*e && *e != ',') break;
        }
        const char *hm = getenv("BZHIP_HUFFMAN");
        if (devices.size() > 1 && !(hm && std::string(hm) == "fixed") && index_path.empty()) { // (an index comes from the streaming path)
            std::vector<uint8_t> data;
            std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)16 << 20]);
            for (;;) {
                const size_t k = fread(buf.get(), 1, (size_t)16 << 20, inf);
                data.insert(data.end(), buf.get(), buf.get() + k);
                if (k < ((size_t)16 << 20)) {
                    if (ferror(inf)) die(ERR_OUTPUT, "error during compression: read failed");
                    break;
                }
            }
            bzh_multi *m = nullptr;
            int ms = bzh_create_multi(&m, devices.data(), (int)devices.size(), level);
            if (ms != BZH_OK) die(ERR_OUTPUT, std::string("error during compression: ") + bzh_strerror(ms));
            const size_t n = data.size(), cap = n + n / 4 + (n / 70000 + 4) * 4096 + 65536;
            std::unique_ptr<uint8_t[]> out(new (std::nothrow) uint8_t[cap]);
            size_t got = 0;
            static const uint8_t none = 0;
            ms = out ? bzh_multi_encode(m, n ? data.data() : &none, n, out.get(), cap, &got, nullptr) : BZH_E_NOMEM;
            if (ms != BZH_OK) {
                const std::string msg = std::string("error during compression: ") + bzh_strerror(ms) + ": " + bzh_multi_last_error(m);
                bzh_destroy_multi(m);
                die(ERR_OUTPUT, msg);
            }
            bzh_destroy_multi(m);
            if (got && fwrite(out.get(), 1, got, outf) != got) die(ERR_OUTPUT, "error during compression: write failed");
            if (!in_stdin) fclose(inf);
            if (fflush(outf) != 0) die(ERR_OUTPUT, "error during compression: write failed");
            if (outf != stdout) fclose(outf);
            const bool keep_in = keep >= 0 ? keep == 1 : have_out; // bnz/src/main.rs:292-300
            if (!keep_in && !in_stdin && remove(in_path.c_str()) != 0)
                die(ERR_OUTPUT, "error deleting input file: " + std::string(strerror(errno)));
            return SUCCESS;
        }
    }
    const char *devs = getenv("BZHIP_DEVICE");
    bzh_ctx *ctx = nullptr;
    int st = bzh_create(&ctx, devs ? atoi(devs) : 0, level, 0);
    if (st != BZH_OK) die(ERR_OUTPUT, std::string("error during compression: ") + bzh_strerror(st));
    auto fail = [&](const std::string &what) {
        const std::string msg = "error during compression: " + what;
        bzh_destroy(ctx);
        die(ERR_OUTPUT, msg);
    };
    // not a flag: the reference's option grammar stays as it is.  BZHIP_HUFFMAN=fixed selects the opt-in Huffman mode
    // (2..6 tables, real refinement: smaller files that are no longer bit-identical to banzai's)
    const char *hm = getenv("BZHIP_HUFFMAN");
    if (hm && std::string(hm) == "fixed") {
        st = bzh_set_mode(ctx, BZH_MODE_FIXED);
        if (st != BZH_OK) fail(bzh_strerror(st));
    }
    const bool with_index = !index_path.empty();
    st = with_index ? bzh_stream_begin_index(ctx, interval) : bzh_stream_begin(ctx);
    if (st != BZH_OK) fail(bzh_strerror(st));
    // --index: what every feed made final is taken at once, so the library holds one pass's worth; the whole index waits here
    // and is written once, at the end (the file's header holds the counts and a CRC over everything)
    std::vector<bzh_index_entry> ix_ent;
    std::vector<bzh_sync_point> ix_pts;
    uint64_t written = 0;
    const size_t CHUNK = (size_t)16 << 20;
    // plain arrays, not vectors: the output bound is a worst case of a few hundred megabytes of which a feed fills a
    // fraction -- value-initialising it (and copying it when it grows) cost more than encoding a 100 MB file
    std::unique_ptr<uint8_t[]> in(new uint8_t[CHUNK]), out;
    size_t out_cap = 0;
    for (bool eof = false; !eof;) {
        const size_t k = fread(in.get(), 1, CHUNK, inf);
        if (k < CHUNK) {
            if (ferror(inf)) fail("read failed");
            eof = true;
        }
        const size_t cap = bzh_stream_bound(ctx, k); // depends on what is pending and in flight: ask every time
        if (out_cap < cap) {
            out.reset(); // (nothing in it is still needed)
            out_cap = cap + cap / 2;
            out.reset(new (std::nothrow) uint8_t[out_cap]);
            if (!out) fail("out of memory");
        }
        size_t got = 0;
        st = bzh_stream_feed(ctx, in.get(), k, eof ? 1 : 0, out.get(), out_cap, &got);
        if (st != BZH_OK) fail(std::string(bzh_strerror(st)) + ": " + bzh_last_error(ctx));
        if (got && fwrite(out.get(), 1, got, outf) != got) fail("write failed");
        written += got;
        if (with_index) {
            size_t ne = 0, np = 0;
            st = bzh_stream_index_pending(ctx, &ne, &np);
            if (st != BZH_OK) fail(bzh_strerror(st));
            const size_t e0 = ix_ent.size(), p0 = ix_pts.size();
            ix_ent.resize(e0 + ne);
            ix_pts.resize(p0 + np);
            st = bzh_stream_index_take(ctx, ix_ent.data() + e0, ne, &ne, ix_pts.data() + p0, np, &np);
            if (st != BZH_OK) fail(std::string(bzh_strerror(st)) + ": " + bzh_last_error(ctx));
        }
    }
    bzh_destroy(ctx);
    if (with_index) {
        const std::string bad = write_index(index_path, ix_ent, ix_pts, interval, written);
        if (!bad.empty()) die(ERR_FILESYSTEM, "[filesystem error] " + bad);
    }
    if (!in_stdin) fclose(inf);
    if (fflush(outf) != 0) die(ERR_OUTPUT, "error during compression: write failed");
    if (outf != stdout) fclose(outf);

    const bool keep_input = keep >= 0 ? keep == 1 : have_out; // bnz/src/main.rs:292-300
    if (!keep_input && !in_stdin && remove(in_path.c_str()) != 0)
        die(ERR_OUTPUT, "error deleting input file: " + std::string(strerror(errno)));
    return SUCCESS;
}
